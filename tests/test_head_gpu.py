"""GPU parity of the HIP head (through the C ABI) against the reference-generated golden fixtures and the oracle.

Tolerances (north_star: score maps within 1e-4 fp32) live in tests/util.py:
  cls      1e-5 absolute  (values ~0.3-0.45; measured ~3e-7)
  loc      1e-4 absolute + 1e-5 relative (values up to ~1 near the identity; measured ~3e-6)
  corners  2e-3 absolute + 2e-6 relative (pixel coordinates up to ~600; fp32 ulp there is 6e-5; measured ~1e-4)
"""
import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

TOL_CLS, TOL_LOC, TOL_CORNERS = util.TOL_CLS, util.TOL_LOC, util.TOL_CORNERS


PRECISIONS = ["f32", "f16x3", "f16x2", "fft", "fftx3", "fft32"]     # every arithmetic mode must meet the same tolerances


@pytest.fixture(autouse=True)
def _fft_mode_for_any_batch(monkeypatch):
    """precision="fft" hands small class batches to the direct kernel (FFT_MIN_PAIRS); the parity tests want the
    frequency-domain path itself, whatever the batch."""
    from os2d_amd.modeling import head as head_mod
    monkeypatch.setattr(head_mod, "FFT_MIN_PAIRS", 1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", util.head_fixture_names())
def test_head_matches_reference_golden(name, precision, device):
    fx = util.load_head_fixture(name)
    creator = util.make_head_creator(fx["P"], fx["inverse"], fx["state"], device)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in fx["class_fms"]])
        loc, cls, cls_det, corners = head(fx["fm"].to(device), precision=precision)
    torch.cuda.synchronize()
    assert cls_det is cls
    assert loc.shape == fx["ref_loc"].shape and cls.shape == fx["ref_cls"].shape and corners.shape == fx["ref_corners"].shape
    if "ref_q15" in fx:
        assert util.maxdiff(head.class_feature_maps, fx["ref_q15"]) < 1e-6
    # f16x2 (opt-in) rounds the 7x7 layer's weights to fp16: its ~1e-5 parameter error is amplified by the strongly
    # deforming transforms of the x_* fixtures (1 / 0.25 scale inverses, 4x zooms) - still inside north_star's 1e-4 on scores
    scale = 10.0 if (precision == "f16x2" and name.startswith("x_")) else 1.0
    util.assert_head_outputs_close(name, loc, cls, corners, fx["ref_loc"], fx["ref_cls"], fx["ref_corners"], scale=scale)
    if precision in util.FP32_EQUIVALENT:      # per-fixture pins at 3x the error measured on an MI355X (tests/golden/head_fixture_pins.json)
        util.check_or_record_fixture_pin(name, precision, util.head_error_ratios(name, loc, cls, corners, fx["ref_loc"], fx["ref_cls"],
                                                                                 fx["ref_corners"]))
    assert head.range_status(synchronize=True) == 0


def _oracle(fm, class_fms, state, inverse):
    from oracle import head_oracle as O
    with torch.no_grad():
        return O.head_forward(fm, O.prepare_class_maps(class_fms), state, inverse)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("P,inverse", [(6, True), (4, False)])
def test_full_size_matches_oracle(P, inverse, precision, device):
    """BASELINE.json sizes: C=1024, 60x80 feature map (1280x960 input); 2 classes so the oracle takes seconds."""
    from os2d_amd.utils import synthetic
    state = synthetic.make_transform_net_state(P, seed=1)
    fm = synthetic.make_feature_map(1024, 60, 80, seed=0)
    class_fms = synthetic.make_class_feature_maps(2, 1024, sizes=[(15, 15), (13, 17)], seed=1000)
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        loc, cls, _, corners = head(fm.to(device), precision=precision)
    ref = _oracle(fm, class_fms, state, inverse)
    assert util.maxdiff(cls, ref[1]) < TOL_CLS
    assert util.maxdiff(loc, ref[0]) < TOL_LOC
    if precision in util.FP32_EQUIVALENT:         # every mode but the opt-in f16x2: pinned at 3x the measured error
        assert util.maxdiff(cls, ref[1]) < util.PIN_CLS and util.maxdiff(loc, ref[0]) < util.PIN_LOC
        # corners: 1.2e-4 px measured (one fp32 ulp of a coordinate near 1400 px) - pinned at 5x that
        assert util.maxdiff(corners, ref[3]) < 6e-4
    else:
        assert util.maxdiff(corners, ref[3]) < 5e-3   # f16x2 (opt-in): loc within 5e-5 -> a few 1e-3 px at 240-px boxes


@pytest.mark.parametrize("precision", PRECISIONS)
def test_image_batch_chunking_and_cat(precision, device, monkeypatch):
    """A=2 images, 5 classes, workspace capped so that classes go through in several chunks; per-class heads
    concatenated with Os2dHead.cat give the same result as one batched head."""
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=7)
    fm = synthetic.make_feature_map(32, 9, 14, seed=5, A=2)
    class_fms = synthetic.make_class_feature_maps(5, 32, sizes=[(15, 15), (14, 16), (16, 14)], seed=500)
    creator = util.make_head_creator(P, inverse, state, device)
    ref = _oracle(fm, class_fms, state, inverse)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        head.precision = precision
        out_full = head(fm.to(device))
        # cap the workspace at ~2 classes per chunk
        import ctypes
        from os2d_amd import _lib
        two = ctypes.c_size_t()
        _lib.check(_lib.load().os2d_head_workspace_bytes(2, 2, 32, 9, 14, P, ctypes.byref(two)), "ws")
        head_mod.release_workspaces()
        with monkeypatch.context() as m:
            m.setattr(head_mod, "workspace_cap_bytes", lambda: two.value)
            out_chunked = head(fm.to(device))
        head_mod.release_workspaces()
        singles = [creator.create_os2d_head([c.to(device)]) for c in class_fms]
        out_cat = head_mod.Os2dHead.cat(singles)(fm.to(device), precision=precision)
    for i, tol in ((0, TOL_LOC), (1, TOL_CLS), (3, TOL_CORNERS)):
        assert util.maxdiff(out_full[i], ref[i]) < tol
        assert util.maxdiff(out_chunked[i], out_full[i]) == 0.0
        assert util.maxdiff(out_cat[i], out_full[i]) == 0.0


ROUTE_SHAPES = {"9x14": (2, 5, 9, 14), "5x212": (1, 3, 5, 212)}      # A, B, H, W at C = 32, P = 6; 5 x 212: wider than the direct kernels, tiled in x
_route_heads = {}


def _route_head(shape, device):
    """(head, feature maps) of a shape, built once for all its precisions"""
    if shape not in _route_heads:
        A, B, H, W = ROUTE_SHAPES[shape]
        state, class_fms, fm = util.route_head_inputs(A, B, H, W)
        creator = util.make_head_creator(6, True, state, device)
        with torch.no_grad():
            head = creator.create_os2d_head([c.to(device) for c in class_fms])
        _route_heads[shape] = head, fm.to(device)
    return _route_heads[shape]


def _forward_ex2(head, fm, precision, workspace_bytes):
    """os2d_head_forward_ex2 through ctypes on a zero-filled workspace of exactly that size: (chunk_classes, [loc, cls, corners])"""
    ws = torch.zeros(workspace_bytes, dtype=torch.uint8, device=fm.device)
    return util.head_forward_ex2(head, fm, precision, ws)          # (outputs NaN-prefilled: a cell nobody writes is never equal)


@pytest.mark.parametrize("shape,precision", [("9x14", p) for p in PRECISIONS] + [("5x212", p) for p in ("fftx3", "fft", "fft32")])
def test_size_entry_point_and_forward_call_carve_the_same_workspace(shape, precision, device):
    """What os2d_head_workspace_bytes_ex reports is what os2d_head_forward_ex2 carves (both go through one route record in abi.hip;
    Os2dHead.forward passes chunk_classes = NULL, so nothing else sees it): a workspace of exactly the reported size takes all B
    classes in one chunk, 256 bytes less - one unit of the carve's alignment - no longer does, the size reported for 2 classes
    gives chunks of exactly 2, and the chunking changes no bit of the outputs."""
    import ctypes
    from os2d_amd import _lib
    from os2d_amd.modeling import head as head_mod
    head, fm = _route_head(shape, device)
    A, B, H, W = ROUTE_SHAPES[shape]
    full, two = ctypes.c_size_t(), ctypes.c_size_t()
    for classes, n in ((B, full), (2, two)):
        _lib.check(_lib.load().os2d_head_workspace_bytes_ex(A, classes, 32, H, W, 6, head_mod.PRECISIONS[precision], ctypes.byref(n)), "ws")
    with torch.no_grad():
        (c_full, o_full), (c_less, o_less), (c_two, o_two) = [_forward_ex2(head, fm, precision, n) for n in (full.value, full.value - 256, two.value)]
    print("chunk_classes {}: {} B -> {}, {} B -> {}, {} B -> {}".format(precision, full.value, c_full, full.value - 256, c_less, two.value, c_two))
    assert c_full == B
    assert 1 <= c_less < B
    assert c_two == 2
    for a, b, c in zip(o_full, o_less, o_two):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["v2_affine_inv", "v1_simple", "v2_c256_wide"])
def test_transformation_net_stage_kernels(name, precision, device):
    """Stage-level parity of the convolution kernels of EVERY arithmetic mode: TransformationNet.forward = standalone input
    normalisation + the three conv kernels (f32: os2d_corr_normalize + os2d_transform_conv; f16x3 / f16x2:
    os2d_corr_normalize_f16x3 + os2d_transform_conv_f16x3 - exactly the kernels the fused head launches) on the
    reference's own correlation tensor, against the TransformNet parameters the reference computed from it."""
    from oracle import head_oracle as O
    fx = util.load_head_fixture(name)
    creator = util.make_head_creator(fx["P"], fx["inverse"], fx["state"], device)
    net = creator.aligner.parameter_regressor
    with torch.no_grad():
        p = net(fx["ref_corr"].to(device), precision=precision)
    tol = 1e-5 if precision != "f16x2" else 1e-4       # f16x2 rounds the 7x7 weights to fp16
    assert util.maxdiff(p, fx["ref_params"]) < tol
    assert util.maxdiff(p, O.transform_net(fx["ref_corr"], fx["state"])) < tol
    if precision not in ("f32", "fft32"):
        assert int(net.last_status.item()) == 0


@pytest.mark.parametrize("name", ["v2_affine_inv", "v1_simple", "x_rot90_inv", "x_scale_inv", "x_near_singular_inv"])
def test_alignment_forward_returns_the_reference_grids(name, device):
    """Os2dAlignment.forward / prepare_transform_parameters_for_grid_sampler as the reference returns them
    (head.py:81-193): theta [N*H*W,2,3] and the template grids [N,H,W,15,15,2] in local coordinates, against the oracle's
    restatement evaluated on the reference's own TransformNet parameters."""
    import torch.nn.functional as F
    from oracle import head_oracle as O
    fx = util.load_head_fixture(name)
    creator = util.make_head_creator(fx["P"], fx["inverse"], fx["state"], device)
    params = fx["ref_params"]
    theta_ref = O.params_to_theta(params, fx["inverse"])
    grids_ref = F.affine_grid(theta_ref, [theta_ref.size(0), 1, 15, 15], align_corners=True)
    N, _, H, W = params.shape
    with torch.no_grad():
        theta = creator.aligner.prepare_transform_parameters_for_grid_sampler(params.to(device))
        _, grids = creator.aligner._grids(params.to(device), False, True)
    assert tuple(theta.shape) == (N * H * W, 2, 3) and tuple(grids.shape) == (N, H, W, 15, 15, 2)
    util.assert_close(theta, theta_ref, 1e-6, 2e-6, name + " theta")
    util.assert_close(grids.view(-1, 15, 15, 2), grids_ref, 2e-6, 3e-6, name + " grids")
    if "ref_corr" in fx:      # the whole module: correlation in, grids out
        with torch.no_grad():
            g2 = creator.aligner(fx["ref_corr"].to(device))
        util.assert_close(g2.view(-1, 15, 15, 2), grids_ref, 2e-5, 1e-5, name + " forward")


def test_cpu_tensors_fail_loudly(device):
    fx = util.load_head_fixture("v1_simple")
    creator = util.make_head_creator(fx["P"], fx["inverse"], fx["state"], device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        creator.create_os2d_head(fx["class_fms"])          # CPU class maps
    head = creator.create_os2d_head([c.to(device) for c in fx["class_fms"]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(fx["fm"])                                      # CPU feature map


def test_singular_transform_is_regularised_locally(device):
    """use_inverse_geom_model with an exactly singular matrix at ONE location: torch.inverse raises and the reference
    retries the whole 65535-matrix chunk with +1e-5 on the diagonal (head.py:125-134); we regularise only the singular
    matrix.  All other locations must be untouched and the singular one finite and equal to the
    regularised closed form."""
    import ctypes
    from os2d_amd import _lib
    lib = _lib.load()
    H, W, P = 5, 6, 6
    HW = H * W
    g = torch.Generator().manual_seed(1)
    corr = torch.rand(1, 225, HW, generator=g)
    params = torch.zeros(1, P, HW)
    params[0, 0], params[0, 4] = 1.0, 1.0                      # identity everywhere
    params[0, :, 7] = torch.tensor([2.0, 4.0, 0.3, 1.0, 2.0, -0.2])   # det = 2*2 - 4*1 = 0 at location 7
    outs = []
    for p in (params, params.clone()):
        loc = torch.empty(1, 4, HW, device=device)
        cls = torch.empty(1, 1, HW, device=device)
        corners = torch.empty(1, 8, HW, device=device)
        _lib.check(lib.os2d_sample_decode(_lib.ptr(corr.to(device)), _lib.ptr(p.to(device)), 1, H, W, P, 1, 16, 16,
                                          _lib.ptr(loc), _lib.ptr(cls), _lib.ptr(corners), _lib.current_stream(device)), "sample")
        outs.append((loc.cpu(), cls.cpu(), corners.cpu()))
        p[0, :, 7] = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])   # second run: identity there too
    (loc_s, cls_s, cor_s), (loc_i, cls_i, cor_i) = outs
    assert torch.isfinite(loc_s).all() and torch.isfinite(cls_s).all() and torch.isfinite(cor_s).all()
    others = [i for i in range(HW) if i != 7]
    assert torch.equal(loc_s[..., others], loc_i[..., others]) and torch.equal(cls_s[..., others], cls_i[..., others])
    # regularised closed form at the singular location: inverse of [[a+e, b, tx],[c, d+e, ty],[0,0,1+e]]
    e = 1e-5
    M = torch.tensor([[2.0 + e, 4.0, 0.3], [1.0, 2.0 + e, -0.2], [0.0, 0.0, 1.0 + e]], dtype=torch.float64)
    Minv = torch.inverse(M)[:2]
    h, w = 7 // W, 7 % W
    expect = [120 * float(Minv[0] @ torch.tensor([x, y, 1.0], dtype=torch.float64)) + 16 * (w + 0.5) for y in (-1, 1) for x in (-1, 1)]
    got = cor_s[0, 0::2, 7].double().tolist()
    # condition number ~1e5: fp32 evaluation of the regularised inverse is good to ~1e-3 relative
    assert max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(got, expect)) < 1e-2


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,H,W,B", [(12, 2, 3, 1), (20, 3, 2, 2), (8, 7, 1 + 4, 3), (36, 33, 40, 2), (1, 4, 5, 2), (7, 5, 4, 3), (13, 9, 11, 2),
                                     (33, 12, 10, 7)])
def test_odd_shapes_match_oracle(C, H, W, B, precision, device):
    """Tiny / ragged shapes: C not a multiple of 8 (half-empty channel group), maps smaller than one tile, a single
    class, a map spanning several tiles with a ragged last one."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=31)
    # +0.05: with so few channels relu(randn) produces all-zero feature vectors; x / (||x|| + 1e-5) at such a cell
    # amplifies the 1e-7 round-off of the 15x15 bilinear resize into O(1e-2) differences in BOTH implementations
    # (an ill-conditioned input, not a property of the kernels) - keep the vectors away from exact zero here
    fm = synthetic.make_feature_map(C, H, W, seed=41) + 0.05
    class_fms = [c + 0.05 for c in synthetic.make_class_feature_maps(B, C, sizes=[(15, 15), (11, 19)], seed=900)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        loc, cls, _, corners = head(fm.to(device), precision=precision)
    ref = _oracle(fm, class_fms, state, inverse)
    assert util.maxdiff(cls, ref[1]) < TOL_CLS
    assert util.maxdiff(loc, ref[0]) < TOL_LOC
    assert util.maxdiff(corners, ref[3]) < TOL_CORNERS


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_size_class_batch_invariance(precision, device):
    """Size-independent property at BASELINE.json's full size (C=1024, 60x80): a class's outputs do not depend on which
    other classes share the batch, nor on the class order (the kernels shard work by class)."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=1)
    fm = synthetic.make_feature_map(1024, 60, 80, seed=0).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(6, 1024, seed=1000)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        full = creator.create_os2d_head(class_fms)(fm, precision=precision)
        part = creator.create_os2d_head(class_fms[4:] + class_fms[1:3])(fm, precision=precision)   # classes 4,5,1,2
    for i in (0, 1, 3):
        assert torch.equal(part[i][:, 0:2], full[i][:, 4:6]) and torch.equal(part[i][:, 2:4], full[i][:, 1:3])
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all() and torch.isfinite(full[3]).all()
    assert float(full[1].min()) > 0.2 and float(full[1].max()) < 0.6      # post-ReLU features: scores 0.3-0.45


@pytest.mark.parametrize("precision", PRECISIONS)
def test_baseline_config_256_classes_v1_properties(precision, device):
    """BASELINE.json configs[3] size (256 classes, V1 head, 1024x60x80) through size-independent properties:
    * both inputs are L2-normalised by the head (reference head.py:293,339), so scaling the image features by 3 and
      the class features by 0.25 (exact power of two / small odd factor) leaves every output unchanged to round-off;
    * a class repeated in the batch gives bit-identical rows wherever it sits (first, middle, last chunk);
    * the 256-class run equals the 64-class runs of its four quarters bit for bit (class chunking / XCD work mapping
      do not leak between classes)."""
    from os2d_amd.utils import synthetic
    P, inverse, B = 4, False, 256
    state = synthetic.make_transform_net_state(P, seed=2)
    fm = synthetic.make_feature_map(1024, 60, 80, seed=3).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(B, 1024, seed=2000)]
    class_fms[100] = class_fms[0]
    class_fms[255] = class_fms[0]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head(class_fms)
        full = head(fm, precision=precision)
        for i in (0, 1, 3):
            assert torch.equal(full[i][:, 0], full[i][:, 100]) and torch.equal(full[i][:, 0], full[i][:, 255])
        for q in range(4):
            part = creator.create_os2d_head(class_fms[64 * q:64 * (q + 1)])(fm, precision=precision)
            for i in (0, 1, 3):
                assert torch.equal(part[i], full[i][:, 64 * q:64 * (q + 1)])
        scaled = creator.create_os2d_head([c * 0.25 for c in class_fms])(fm * 3.0, precision=precision)
    assert util.maxdiff(scaled[1], full[1]) < TOL_CLS
    assert util.maxdiff(scaled[0], full[0]) < TOL_LOC
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[3]).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_widest_supported_level_and_clean_failure_beyond(precision, device):
    """W = 209 columns (a 3344-px wide image) is the widest level the DIRECT 7x7 kernels take; the reference has no width limit
    (head.py:619) and evaluates one class at a time (evaluate.py:226), so beyond it - here W = 260, B = 1 -
    the layer runs in the frequency domain, tiled, whatever the class batch, in the arithmetic family that was asked for; W = 316
    is the widest map of the 5x5 kernels' linear slabs."""
    from os2d_amd.utils import synthetic
    P, inverse, C = 6, True, 16
    state = synthetic.make_transform_net_state(P, seed=4)
    class_fms = [c + 0.05 for c in synthetic.make_class_feature_maps(2, C, sizes=[(15, 15), (14, 16)], seed=77)]
    creator = util.make_head_creator(P, inverse, state, device)
    for W, B in ((209, 2), (260, 1), (316, 2)):
        fm = synthetic.make_feature_map(C, 9, W, seed=5) + 0.05
        with torch.no_grad():
            head = creator.create_os2d_head([c.to(device) for c in class_fms[:B]])
            loc, cls, _, corners = head(fm.to(device), precision=precision)
        if W > 209:        # the direct families took the frequency-domain route of their arithmetic
            assert head.last_precision == {"f32": "fft32", "f16x3": "fftx3", "f16x2": "fftx3"}.get(precision, precision)
        ref = _oracle(fm, class_fms[:B], state, inverse)
        assert util.maxdiff(cls, ref[1]) < TOL_CLS, W
        assert util.maxdiff(loc, ref[0]) < TOL_LOC, W
        assert util.maxdiff(corners, ref[3]) < 1.2e-2, W      # coordinates up to ~5000 px


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("W,H", [(317, 6), (400, 9), (640, 7), (1030, 3)])
def test_maps_wider_than_the_linear_slabs_run_in_column_strips(W, H, precision, device):
    """the reference has no width limit (head.py:619-629).  Beyond W = 316 the 5x5 kernels run in column
    strips (conv_f16x3.hip STRIP mode, conv3_f16x3.hip, conv_mfma.hip; geometry restated in tests/test_conv_strips_model.py) and
    the 7x7 layer in the tiled frequency domain - parity at B = 1 and B = 8 in every arithmetic mode, V2 and V1 heads, and the
    1-class call equals the slice of the 8-class call bit for bit."""
    from os2d_amd.utils import synthetic
    C = 16
    for P, inverse in ((6, True), (4, False)):
        state = synthetic.make_transform_net_state(P, seed=4 + P)
        class_fms = [c + 0.05 for c in synthetic.make_class_feature_maps(8, C, sizes=[(15, 15), (14, 16), (17, 13)], seed=78)]
        creator = util.make_head_creator(P, inverse, state, device)
        fm = synthetic.make_feature_map(C, H, W, seed=W) + 0.05
        ref = _oracle(fm, class_fms, state, inverse)
        with torch.no_grad():
            head8 = creator.create_os2d_head([c.to(device) for c in class_fms])
            loc8, cls8, _, cor8 = head8(fm.to(device), precision=precision)
            head1 = creator.create_os2d_head([class_fms[3].to(device)])
            loc1, cls1, _, cor1 = head1(fm.to(device), precision=precision)
        assert head8.last_precision == {"f32": "fft32", "f16x3": "fftx3", "f16x2": "fftx3"}.get(precision, precision)
        assert util.maxdiff(cls8, ref[1]) < TOL_CLS and util.maxdiff(loc8, ref[0]) < TOL_LOC, (W, P)
        assert util.maxdiff(cor8, ref[3]) < 2.5e-2, (W, P)      # coordinates up to ~10,000 px
        assert util.maxdiff(cls1, ref[1][:, 3:4]) < TOL_CLS and util.maxdiff(loc1, ref[0][:, 3:4]) < TOL_LOC, (W, P)
        assert torch.equal(loc1, loc8[:, 3:4]) and torch.equal(cls1, cls8[:, 3:4]) and torch.equal(cor1, cor8[:, 3:4]), (W, P)


def test_clean_failure_beyond_the_planner_width(device):
    """Beyond OS2D_MAX_W = 3600 columns (57,600-px images) the head fails, loudly and BEFORE anything is launched."""
    from os2d_amd.utils import synthetic
    state = synthetic.make_transform_net_state(6, seed=4)
    creator = util.make_head_creator(6, True, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in synthetic.make_class_feature_maps(1, 16, sizes=[(15, 15)], seed=7)])
        with pytest.raises(RuntimeError, match="width"):
            head(torch.zeros(1, 16, 2, 3601, device=device))


def test_clean_failure_beyond_the_planner_height(device):
    """beyond OS2D_MAX_H = 2784 rows (48 tiles of 58) the head fails in the argument check, not inside the planner."""
    from os2d_amd.utils import synthetic
    state = synthetic.make_transform_net_state(6, seed=4)
    creator = util.make_head_creator(6, True, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in synthetic.make_class_feature_maps(1, 16, sizes=[(15, 15)], seed=7)])
        with pytest.raises(RuntimeError, match="height"):
            head(torch.zeros(1, 16, 2785, 3, device=device))


@pytest.mark.parametrize("precision", [None, "fft32"])
@pytest.mark.parametrize("W,H", [(3600, 2), (3, 2784), (700, 130)])
def test_maps_at_the_planner_limits(W, H, precision, device):
    """strip mode and tiling were tested to W = 1030 only.  The widest map (48 transform tiles, 15 column strips), the
    tallest (48 tiles along H, strip planes of 2784 rows) and a map tiled on both axes at once, against the oracle.  Corners are
    coordinates of up to 57,600 px: their tolerance is relative (one fp32 ulp there is 4e-3 px)."""
    from os2d_amd.utils import synthetic
    C = 8
    state = synthetic.make_transform_net_state(6, seed=10)
    class_fms = [c + 0.05 for c in synthetic.make_class_feature_maps(2, C, sizes=[(15, 15), (13, 17)], seed=79)]
    creator = util.make_head_creator(6, True, state, device)
    fm = synthetic.make_feature_map(C, H, W, seed=W + H) + 0.05
    ref = _oracle(fm, class_fms, state, True)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        loc, cls, _, cor = head(fm.to(device), precision=precision)
    assert head.last_precision == (precision or "fftx3")
    # (2- and 3-cell wide maps: every template hangs over the border and the clamped sampling amplifies the parameters' last bits -
    # the strict-fp32 mode shows the same 1.6e-4 on loc as the default one - so loc and corners get their relative terms)
    util.assert_head_outputs_close("limits", loc, cls, cor, ref[0], ref[1], ref[3], scale=2.0, corners_scale=16.0 * max(W, H) / 1400.0)


def _random_shapes(n, seed):
    rs = np.random.RandomState(seed)
    shapes = [(4, 1, 1, 1, 1, 6, True), (8, 1, 64, 1, 2, 4, False), (4, 37, 1, 2, 1, 6, False)]      # degenerate maps first
    while len(shapes) < n:
        shapes.append((int(rs.randint(1, 17)) * 4, int(rs.randint(1, 41)), int(rs.randint(1, 61)), int(rs.randint(1, 3)),
                       int(rs.randint(1, 10)), int(rs.choice([4, 6])), bool(rs.randint(0, 2))))
    # channel counts that are NOT a multiple of 4 (round 6: any C, as in the reference): a second stream, so that the shapes above keep
    # their values
    rs2 = np.random.RandomState(seed + 1)
    for _ in range(4):
        shapes.append((int(rs2.randint(1, 70)) | 1, int(rs2.randint(1, 41)), int(rs2.randint(1, 61)), int(rs2.randint(1, 3)),
                       int(rs2.randint(1, 10)), int(rs2.choice([4, 6])), bool(rs2.randint(0, 2))))
    return shapes


@pytest.mark.parametrize("C,H,W,A,B,P,inverse", _random_shapes(14, seed=2024))
def test_random_shapes_all_precisions_match_oracle(C, H, W, A, B, P, inverse, device):
    """Seeded sweep over channel counts (multiples of 4 and odd ones), map sizes from 1x1 to 40x60 (partial tiles, single rows /
    columns), image batches and class counts, both head variants: every arithmetic mode against the oracle."""
    from os2d_amd.utils import synthetic
    state = synthetic.make_transform_net_state(P, seed=C + H)
    fm = synthetic.make_feature_map(C, H, W, seed=H * 100 + W, A=A) + 0.05
    class_fms = [c + 0.05 for c in synthetic.make_class_feature_maps(B, C, sizes=[(15, 15), (9, 23), (16, 14)], seed=B * 7 + C)]
    creator = util.make_head_creator(P, inverse, state, device)
    ref = _oracle(fm, class_fms, state, inverse)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        for precision in PRECISIONS:
            loc, cls, _, corners = head(fm.to(device), precision=precision)
            assert tuple(loc.shape) == (A, B, 4, H, W) and tuple(cls.shape) == (A, B, 1, H, W)
            assert util.maxdiff(cls, ref[1]) < TOL_CLS, precision
            assert util.maxdiff(loc, ref[0]) < TOL_LOC, precision
            assert util.maxdiff(corners, ref[3]) < TOL_CORNERS, precision


@pytest.mark.parametrize("precision", PRECISIONS)
def test_small_batches_equal_slices_of_a_large_batch(precision, device):
    """A handful of classes runs through finer work-group shapes than a large batch (128-position tiles, 32 output
    channels per group); every output element still accumulates the same products in the same order, so a 1-, 2- or
    5-class call equals the corresponding slice of a 40-class call bit for bit - at the full 1024 x 60 x 80 size."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=8)
    fm = synthetic.make_feature_map(1024, 60, 80, seed=9).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(40, 1024, sizes=[(15, 15), (13, 17)], seed=3000)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        big = creator.create_os2d_head(class_fms)(fm, precision=precision)
        for lo, hi in ((0, 1), (17, 19), (30, 35)):
            small = creator.create_os2d_head(class_fms[lo:hi])(fm, precision=precision)
            for i in (0, 1, 3):
                assert torch.equal(small[i], big[i][:, lo:hi]), (lo, hi, i)


@pytest.mark.parametrize("B,iters", [(64, 150), (2, 400)])
def test_repeated_calls_are_bit_identical(B, iters, device):
    """Soak test of the asynchronous staging (LDS-DMA in the correlation, register prefetch pipelines in the convolutions,
    both work-group shapes): hundreds of back-to-back calls at the full 1024 x 60 x 80 size must reproduce the first
    result bit for bit - a read that races a DMA or a prefetch shows up as a rare wrong tile."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=12)
    fm = synthetic.make_feature_map(1024, 60, 80, seed=13).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(B, 1024, seed=4000)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head(class_fms)
        first = [t.clone() for t in head(fm)]
        bad = torch.zeros((), dtype=torch.int64, device=device)
        for _ in range(iters):
            out = head(fm)
            for i in (0, 1, 3):
                bad += (out[i] != first[i]).sum()
    assert int(bad) == 0


# ------------------------------------------------------------------------------------------------ range safety
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("P,inverse", [(6, True), (4, False)])
def test_hostile_dynamic_range_network(P, inverse, precision, device):
    """a TransformNet whose folded BatchNorm scales span nine decades between channels
    (1e-3 .. 1e6), running_var = 1e-6, activations from 1e-5 (below 2^-14) to 1e5 (beyond 65504) and weight rows /
    columns with a 2^30 dynamic range - function-preserving rescalings of an ordinary network
    (tests/util.py:adversarial_transform_net_state), so the reference's fp32 arithmetic loses nothing on it.  Every
    arithmetic mode must match the oracle at the usual tolerances, without raising the range flag."""
    from os2d_amd.utils import synthetic
    state = util.adversarial_transform_net_state(P, seed=21)
    fm = synthetic.make_feature_map(64, 14, 19, seed=6)
    class_fms = synthetic.make_class_feature_maps(3, 64, sizes=[(15, 15), (12, 18), (17, 13)], seed=600)
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        loc, cls, _, corners = head(fm.to(device), precision=precision)
    ref = _oracle(fm, class_fms, state, inverse)
    util.assert_head_outputs_close("hostile", loc, cls, corners, ref[0], ref[1], ref[3])
    assert head.range_status(synchronize=True) == 0
    # the same network in its ordinary scaling gives the same outputs (function-preserving rescaling)
    base = util.make_head_creator(P, inverse, synthetic.make_transform_net_state(P, seed=21), device)
    with torch.no_grad():
        loc0, cls0, _, corners0 = base.create_os2d_head([c.to(device) for c in class_fms])(fm.to(device), precision=precision)
    util.assert_head_outputs_close("hostile vs base", loc, cls, corners, loc0, cls0, corners0)


@pytest.mark.parametrize("precision", ["f16x3", "f16x2"])
def test_full_size_hostile_network_matches_f32_mode(precision, device):
    """The hostile network at BASELINE.json's size (C=1024, 60x80, 8 classes): split-fp16 modes against the exact-fp32
    kernels on the benchmarked tensors."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = util.adversarial_transform_net_state(P, seed=1)
    fm = synthetic.make_feature_map(1024, 60, 80, seed=0).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(8, 1024, seed=1000)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head(class_fms)
        ref = [t.clone() for t in head(fm, precision="f32")]
        out = head(fm, precision=precision)
    tol = 1.0 if precision == "f16x3" else 4.0
    util.assert_head_outputs_close(precision, out[0], out[1], out[3], ref[0], ref[1], ref[3], scale=tol)
    assert head.range_status(synchronize=True) == 0


@pytest.mark.parametrize("precision", ["fftx3", "fft", "f16x3"])
def test_nan_feature_map_raises_the_range_flag(precision, device):
    """VERDICT r5 item 5 / ADVICE r5: a NaN in an image feature map.  The reference's torch.relu / norm propagate it (head.py:339,
    650); fmaxf(NaN, 0) = 0 and the fp16 splits of the split-fp16 kernels do not.  Round 5 returned finite numbers for that call
    and ran the NEXT call in fp32.  Now the kernel that normalises the image features raises the range word of the image and the last
    kernel of THE SAME call writes NaN into every output of that image: (i) the flagged call is NaN wherever the oracle is,
    (ii) the other image of the batch is untouched and bit-equal to a clean run, (iii) the following call with finite input is
    bit-identical to a clean run and stays in the configured arithmetic, (iv) ``strict_range`` still gives the exact fp32 run."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=3)
    clean = torch.cat([synthetic.make_feature_map(32, 12, 14, seed=2), synthetic.make_feature_map(32, 12, 14, seed=5)], 0)
    fm = clean.clone()
    fm[1, 5, 3, 4] = float("nan")
    class_fms = synthetic.make_class_feature_maps(8, 32, seed=20)
    creator = util.make_head_creator(P, inverse, state, device)
    ref = _oracle(fm, class_fms, state, inverse)
    assert torch.isnan(ref[1][1]).any() and not torch.isnan(ref[1][0]).any()
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        before = [t.clone() for t in head(clean.to(device), precision=precision)]
        ran = head.last_precision
        assert head.range_status(synchronize=True) == 0
        bad = [t.clone() for t in head(fm.to(device), precision=precision)]
        assert head.last_precision == ran
        assert head.range_status(synchronize=True) == 1            # the sticky host word, raised by the same call
        after = head(clean.to(device), precision=precision)       # the NEXT call: same arithmetic, same bits as before
        assert head.last_precision == ran
        for a, b in zip(after, before):
            assert torch.equal(a, b)
        head.clear_range_status()
        head(clean.to(device), precision=precision)
        assert head.range_status(synchronize=True) == 0            # ... and it does not raise the word again
    for k, (got, want) in enumerate(zip(bad, (ref[0], ref[1], ref[1], ref[3]))):
        got = got.cpu()
        assert torch.isnan(got[1]).all()                          # image 1: NaN everywhere (a superset of the oracle's NaNs)
        assert bool(torch.isnan(got)[torch.isnan(want)].all())
        assert torch.equal(got[0], before[k][0].cpu())            # image 0 of the batch: bit-equal to the clean run
    with torch.no_grad():
        out = head(fm.to(device), precision=precision, strict_range=True)
        assert head.last_precision == "f32"
        plain = creator.create_os2d_head([c.to(device) for c in class_fms])(fm.to(device), precision="f32")
    # (the NaN PATTERN of the reference depends on torch's min / max / grid_sample treatment of NaN coordinates, which fminf /
    # fmaxf in the resampler do not share; what is pinned for strict_range is that the re-run is the exact fp32 path)
    for a, b in zip(out, plain):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def test_range_flag_is_raised_not_clamped(device):
    """Besides non-finite input, weights that make an activation overflow are the only way past the range plan: the split-fp16
    kernels then raise the call's range word instead of clamping silently; the call's outputs are NaN (the reference's are
    non-finite there), the sticky host word is raised (mapped host memory: polled without synchronisation), ``strict_range`` re-runs
    the call in exact fp32, and the next call is NOT affected (round 5 ran it in fp32)."""
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=3)
    # a huge (finite) weight makes conv 7x7 outputs overflow fp32 itself -> inf activations
    state["conv.0.bias"][5] = 3e38
    state["conv.1.weight"][5] = 1e3
    fm = synthetic.make_feature_map(32, 8, 9, seed=2).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(2, 32, seed=20)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head(class_fms)
        head.precision = "f16x3"
        out = head(fm)
        assert head.range_status(synchronize=True) == 1
        assert all(bool(torch.isnan(t).all()) for t in out)
        head(fm)                                   # the next call runs in the configured arithmetic (and is flagged again)
        assert head.last_precision == "f16x3" and head.precision == "f16x3"
        # every head has its OWN word (a shared word let head B consume and clear head A's flag), all of them slots
        # of one per-device array that lives as long as the process (no head owns memory kernels write to)
        other = creator.create_os2d_head(class_fms)
        assert other._status_word().data_ptr() != head._status_word().data_ptr()
        assert 0 < abs(other._status_word().data_ptr() - head._status_word().data_ptr()) < 4 * head_mod.STATUS_SLOTS
        head.clear_range_status()
        head(fm, precision="f16x3")                                           # raises head's flag again ...
        torch.cuda.synchronize()
        assert head.range_status() == 1 and other.range_status() == 0
        other(fm, precision="f32")                                            # ... which a call of ANOTHER head neither sees nor clears
        assert head.range_status(synchronize=True) == 1 and other.range_status() == 0
        head2 = creator.create_os2d_head(class_fms)
        strict = head2(fm, precision="f16x3", strict_range=True)
        assert head2.last_precision == "f32"
        plain = head2(fm, precision="f32")
    for a, b in zip(strict, plain):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0, posinf=7e30, neginf=-7e30), torch.nan_to_num(b, nan=-7.0, posinf=7e30, neginf=-7e30))


def test_route_switch_pin_and_route_pairs(device, monkeypatch):
    """The PRODUCTION route switch (the other tests force FFT_MIN_PAIRS = 1): below 7 (image, class) pairs the frequency-domain
    modes hand the 7x7 layer to the direct kernel; ``precision="fftx3!"`` pins the frequency-domain route and ``route_pairs``
    lets a caller decide on a global pair count (a class-sharded run with a ragged tail rank, os2d_amd/parallel.py) - in both
    cases a 3-class call is then bit-equal to the same classes inside a large batch."""
    from os2d_amd.modeling import head as head_mod
    from os2d_amd.utils import synthetic
    monkeypatch.setattr(head_mod, "FFT_MIN_PAIRS", 7)
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=2)
    fm = synthetic.make_feature_map(64, 21, 26, seed=4).to(device)
    class_fms = [c.to(device) for c in synthetic.make_class_feature_maps(12, 64, sizes=[(15, 15), (14, 16)], seed=90)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        big = creator.create_os2d_head(class_fms)
        ref = big(fm)
        assert big.last_precision == "fftx3"                       # 12 pairs: frequency domain
        small = creator.create_os2d_head(class_fms[9:12])
        plain = [t.clone() if t is not None else None for t in small(fm)]
        assert small.last_precision == "f16x3"                     # 3 pairs: the direct kernel
        pinned = [t.clone() for t in small(fm, precision="fftx3!")]
        assert small.last_precision == "fftx3"
        routed = [t.clone() for t in small(fm, route_pairs=12)]
        assert small.last_precision == "fftx3"
        small.precision = "fftx3!"                                 # ... or as the head's setting
        assert torch.equal(small(fm)[0], pinned[0])
    for i in (0, 1, 3):
        assert torch.equal(pinned[i], ref[i][:, 9:12]) and torch.equal(routed[i], ref[i][:, 9:12])
        assert util.maxdiff(plain[i], ref[i][:, 9:12]) < (1e-5 if i == 1 else 2e-3)      # the two routes agree to the last bits
    with pytest.raises(ValueError):
        small(fm, precision="f16x3!")                              # only the frequency-domain modes have a route to pin


# ------------------------------------------------------------------------------------------------ BASELINE configs[2] / [4]
@pytest.mark.parametrize("B", [128, 1024])
def test_baseline_config_class_counts_128_and_1024(B, device):
    """BASELINE.json configs[2]: 1024 classes at 1024x60x80 (what ONE GPU holds at N=1) and 128 classes (its per-GPU share
    at N=8).  Two classes against the oracle, every class against its own single-class call (slice invariance: the
    XCD-aware work mapping and class chunking do not leak between classes), duplicates bit-identical."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=1)
    fm_cpu = synthetic.make_feature_map(1024, 60, 80, seed=0)
    fm = fm_cpu.to(device)
    base = synthetic.make_class_feature_maps(16, 1024, sizes=[(15, 15), (13, 17), (16, 14)], seed=5000)
    class_cpu = [base[(7 * b) % 16] for b in range(B)]          # 16 distinct classes repeated through the batch
    class_fms = [c.to(device) for c in class_cpu]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head(class_fms)
        loc, cls, _, corners = head(fm)
        ref = _oracle(fm_cpu, [class_cpu[0], class_cpu[B - 1]], state, inverse)
        for k, b in enumerate((0, B - 1)):
            util.assert_head_outputs_close("B{} class {}".format(B, b), loc[:, b], cls[:, b], corners[:, b],
                                           ref[0][:, k], ref[1][:, k], ref[3][:, k], corners_scale=2.5, pin=True)
        # the same class anywhere in the batch -> the same bits
        for b in range(16, B):
            assert torch.equal(cls[:, b], cls[:, b - 16]) and torch.equal(loc[:, b], loc[:, b - 16])
        # 64-class slices equal the big batch bit for bit (first, a middle and the last block)
        for b0 in sorted({0, (B // 2 // 64) * 64, B - 64}):
            part = creator.create_os2d_head(class_fms[b0:b0 + 64])(fm)
            for i in (0, 1, 3):
                assert torch.equal(part[i], (loc, cls, None, corners)[i][:, b0:b0 + 64])
    assert torch.isfinite(loc).all() and torch.isfinite(corners).all()
    assert head.range_status(synchronize=True) == 0


PYRAMID_LEVELS = [(30, 40), (38, 50), (48, 64), (60, 80), (72, 96), (84, 112), (96, 128)]


@pytest.mark.parametrize("H,W", PYRAMID_LEVELS)
def test_baseline_config_pyramid_level_sizes_match_oracle(H, W, device):
    """BASELINE.json configs[4]: every level of the 7-scale pyramid of a 1280x960 image at C = 1024, two classes against
    the oracle (all arithmetic modes)."""
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=1)
    fm = synthetic.make_feature_map(1024, H, W, seed=H)
    class_fms = synthetic.make_class_feature_maps(2, 1024, sizes=[(15, 15), (13, 17)], seed=1000)
    creator = util.make_head_creator(P, inverse, state, device)
    ref = _oracle(fm, class_fms, state, inverse)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        for precision in PRECISIONS:
            loc, cls, _, corners = head(fm.to(device), precision=precision)
            # every level runs the arithmetic it was asked for: the 96 x 128 level takes the frequency-domain route too
            # (overlap-save tiles) - no silent fallback to the direct kernel
            assert head.last_precision == precision
            util.assert_head_outputs_close("{}x{} {}".format(H, W, precision), loc, cls, corners, ref[0], ref[1], ref[3],
                                           scale=1.0 if precision != "f16x2" else 4.0, corners_scale=2.5,    # coordinates up to ~2000 px
                                           pin=precision in util.FP32_EQUIVALENT)


@pytest.mark.parametrize("H,W,C,B,A", [(100, 140, 64, 7, 1), (157, 209, 32, 3, 1), (64, 209, 32, 4, 1), (200, 100, 32, 8, 1), (97, 130, 32, 5, 2)])
def test_tiled_frequency_domain_route_matches_oracle_and_direct_kernel(H, W, C, B, A, device):
    """Maps beyond one in-LDS transform (up to the 209-column limit of the other kernels): the frequency-domain modes cut
    them into overlap-save tiles (os2d_fft_tiles).  Ragged tilings (tile sizes that do not divide the map), a one-axis
    tiling and the widest supported map, against the oracle and against the direct f16x3 kernel on the same inputs."""
    from os2d_amd.utils import synthetic
    from freq_util import fft_tiles
    TY, TX, _, _ = fft_tiles(H, W)
    assert TY * TX > 1, "the case is meant to be tiled"
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=4)
    fm = synthetic.make_feature_map(C, H, W, seed=H + W, A=A)          # A = 2: two images per call (pair = image x class x tile)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=[(15, 15), (12, 18)], seed=77)
    creator = util.make_head_creator(P, inverse, state, device)
    ref = _oracle(fm, class_fms, state, inverse)
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in class_fms])
        direct = [t.clone() for t in head(fm.to(device), precision="f16x3")]
        for precision in ("fft", "fftx3"):
            loc, cls, _, corners = head(fm.to(device), precision=precision)
            assert head.last_precision == precision
            util.assert_head_outputs_close("{}x{} {}".format(H, W, precision), loc, cls, corners, ref[0], ref[1], ref[3], corners_scale=2.5)
            util.assert_head_outputs_close("{}x{} {} vs direct".format(H, W, precision), loc, cls, corners, direct[0], direct[1], direct[3], corners_scale=2.5)


def test_baseline_config_pyramid_streams_128_classes(device):
    """configs[4] per-GPU share: 128 classes over all seven level sizes at C = 1024, one HIP stream per level
    (PyramidHeadRunner) against the same levels run one after the other on one stream - bit-identical, twice (the
    second run reuses the cached operands and the per-stream workspaces)."""
    from os2d_amd.engine.pyramid import PyramidHeadRunner
    from os2d_amd.utils import synthetic
    P, inverse = 6, True
    state = synthetic.make_transform_net_state(P, seed=1)
    levels = [synthetic.make_feature_map(1024, h, w, seed=100 + i).to(device) for i, (h, w) in enumerate(PYRAMID_LEVELS)]
    base = [c.to(device) for c in synthetic.make_class_feature_maps(8, 1024, seed=7000)]
    creator = util.make_head_creator(P, inverse, state, device)
    with torch.no_grad():
        head = creator.create_os2d_head([base[b % 8] for b in range(128)])
        serial = PyramidHeadRunner(head, num_streams=1, device=device).run(levels, inputs_are_features=True)
        torch.cuda.synchronize()
        for _ in range(2):
            par = PyramidHeadRunner(head, num_streams=len(levels), device=device).run(levels, inputs_are_features=True)
            torch.cuda.synchronize()
            for lvl in range(len(levels)):
                for k in range(3):
                    assert torch.equal(par[k][lvl], serial[k][lvl]), (lvl, k)
    from os2d_amd.modeling import head as head_mod
    assert len(head_mod._WORKSPACES) <= len(levels) + 1          # one workspace per level stream (+ the caller's)


# ------------------------------------------------------------------------------------------------ correlation stage
@pytest.mark.parametrize("name", ["v2_affine_inv", "affine_noinv", "v2_c256_wide"])
def test_correlation_stage_matches_reference(name, device):
    """Stage-level parity of BOTH correlation kernels against the correlation tensor the reference computed
    (``ref_corr``, the TransformNet input recorded by a forward hook in tests/golden/make_golden.py): os2d_fm_sumsq +
    os2d_corr (fp32 MFMA) and os2d_corr_f16x3 (split-fp16 MFMA, LDS-DMA staging, wide-store epilogue) through the C ABI;
    their normalised outputs (zero-bordered planes / split-half blocked units) against relu + L2 of the same tensor."""
    import torch.nn.functional as F
    from freq_util import plane_interior, shb_decode
    from os2d_amd import _lib
    lib = _lib.load()
    fx = util.load_head_fixture(name)
    creator = util.make_head_creator(fx["P"], fx["inverse"], fx["state"], device)
    fm = fx["fm"].to(device)
    A, C, H, W = fm.shape
    HW = H * W
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in fx["class_fms"]])
    B = head.class_batch_size
    NB = A * B
    st = _lib.current_stream(device)
    ref = fx["ref_corr"].reshape(NB, 225, HW)
    r = F.relu(fx["ref_corr"])
    rn_ref = (r / (r.norm(dim=1, keepdim=True) + 1e-6)).reshape(NB, 225, H, W)
    plane = lib.os2d_plane_floats(H, W)
    Ws, base = plane_interior(H, W)
    # ---- fp32 kernels
    # (outputs and workspaces pre-filled with NaN / 0xFF bytes: an unwritten cell cannot pass as a zero)
    sumsq = torch.full((A * HW,), float("nan"), device=device)
    corr = torch.full((NB, 225, HW), float("nan"), device=device)
    rnorm = torch.full((NB * 226 * plane,), float("nan"), device=device)
    _lib.check(lib.os2d_fm_sumsq(_lib.ptr(fm), _lib.ptr(sumsq), A, C, H, W, st), "os2d_fm_sumsq")
    _lib.check(lib.os2d_corr(_lib.ptr(fm), _lib.ptr(head._qp), _lib.ptr(sumsq), _lib.ptr(corr), _lib.ptr(rnorm), A, B, C, H, W, st), "os2d_corr")
    assert util.maxdiff(corr, ref) < 2e-6
    got = rnorm.view(NB, 226, plane)[:, :225, base:base + H * Ws].reshape(NB, 225, H, Ws)[..., :W]
    assert util.maxdiff(got, rn_ref) < 2e-6
    # ---- split-fp16 kernels
    nbytes = lib.os2d_corr_f16x3_workspace_bytes(A, C, H, W)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
    corr16 = torch.full((NB, 225, HW), float("nan"), device=device)
    shb_bytes = lib.os2d_shb_bytes(225, H, W)
    rshb = torch.full((NB * shb_bytes,), 0xFF, dtype=torch.uint8, device=device)
    _lib.check(lib.os2d_corr_f16x3(_lib.ptr(fm), _lib.ptr(head._split_class_operand()), _lib.ptr(corr16), _lib.ptr(rshb), A, B, C, H, W,
                                   _lib.ptr(ws), ws.numel(), st), "os2d_corr_f16x3")
    assert util.maxdiff(corr16, ref) < 2e-6
    # split-half blocked units: [NB][29][hi|lo][PLANE][8 halves], value = (hi + lo) * 2^-rnorm_exp
    val, border = shb_decode(rshb, NB, 232, H, W)
    got16 = val[:, :225] * 2.0 ** -lib.os2d_rnorm_exp()
    assert util.maxdiff(got16, rn_ref) < 2e-6
    assert float(val[:, 225:].abs().max()) == 0.0                                              # padding channels of the last group
    assert border == 0.0                                                                       # zero borders baked in


def _packed_corr(lib, fm, qs, B, device, form=1):
    from os2d_amd import _lib
    A, C, H, W = fm.shape
    ws = torch.empty(lib.os2d_corr_f16x3_packed_workspace_bytes(A, B, C, H, W), dtype=torch.uint8, device=device)
    corr = torch.full((A * B, 225, H * W), float("nan"), device=device)
    invn = torch.full((A * B, H * W), float("nan"), device=device)
    _lib.check(lib.os2d_corr_f16x3_packed(_lib.ptr(fm), _lib.ptr(qs), _lib.ptr(corr), _lib.ptr(invn), A, B, C, H, W, form, _lib.ptr(ws), ws.numel(),
                                          _lib.current_stream(device)), "os2d_corr_f16x3_packed")
    return corr, invn


@pytest.mark.parametrize("name", ["v2_affine_inv", "affine_noinv", "v2_c256_wide"])
def test_packed_correlation_stage_matches_reference(name, device):
    """The correlation of the frequency-domain heads (classes packed along the matrix rows) against the
    reference's correlation tensor, its inverse norms against relu + L2 of that tensor (head.py:650), and against the padded
    one-class-per-tile kernel: the correlation values bit for bit (the same products in the same order), the norms to rounding."""
    from os2d_amd import _lib
    lib = _lib.load()
    fx = util.load_head_fixture(name)
    creator = util.make_head_creator(fx["P"], fx["inverse"], fx["state"], device)
    fm = fx["fm"].to(device)
    A, C, H, W = fm.shape
    with torch.no_grad():
        head = creator.create_os2d_head([c.to(device) for c in fx["class_fms"]])
    B = head.class_batch_size
    NB, HW = A * B, H * W
    corr, invn = _packed_corr(lib, fm, head._split_class_operand(), B, device)
    ref = fx["ref_corr"].reshape(NB, 225, HW)
    assert util.maxdiff(corr, ref) < 2e-6
    inv_ref = 1.0 / (torch.relu(fx["ref_corr"].double()).reshape(NB, 225, HW).norm(dim=1) + 1e-6)
    assert float(((invn.double().cpu() - inv_ref).abs() / inv_ref).max()) < 3e-6
    # the padded kernel: same correlation bits
    ws = torch.full((lib.os2d_corr_f16x3_workspace_bytes(A, C, H, W),), 0xFF, dtype=torch.uint8, device=device)
    corr16 = torch.full((NB, 225, HW), float("nan"), device=device)
    rshb = torch.full((NB * lib.os2d_shb_bytes(225, H, W),), 0xFF, dtype=torch.uint8, device=device)
    _lib.check(lib.os2d_corr_f16x3(_lib.ptr(fm), _lib.ptr(head._split_class_operand()), _lib.ptr(corr16), _lib.ptr(rshb), A, B, C, H, W,
                                   _lib.ptr(ws), ws.numel(), _lib.current_stream(device)), "os2d_corr_f16x3")
    assert torch.equal(corr, corr16)


@pytest.mark.parametrize("H,W,C,B", [(60, 80, 256, 23), (13, 17, 64, 70), (30, 40, 128, 9)])
def test_packed_correlation_is_independent_of_the_batch_composition(H, W, C, B, device):
    """A class's correlation AND its inverse norms are the same bits whether it is computed alone, at another position of the
    batch or in a sub-batch: the packed kernel's per-position sums cross work-groups as fixed-point integers, so neither the
    alignment of a class inside a row tile nor the order of the atomics can show.  Also: exact against float64 sums of the
    kernel's own correlation values (the fixed point drops < 2^-44 per group of four rows), and a map whose H*W is not a
    multiple of 4 (scalar store path)."""
    from os2d_amd import _lib
    from os2d_amd.utils import synthetic
    lib = _lib.load()
    P = 6
    creator = util.make_head_creator(P, True, synthetic.make_transform_net_state(P, seed=2), device)
    fm = synthetic.make_feature_map(C, H, W, seed=11).to(device)
    cls = [c.to(device) for c in synthetic.make_class_feature_maps(B, C, seed=77)]
    with torch.no_grad():
        head = creator.create_os2d_head(cls)
        corr, invn = _packed_corr(lib, fm, head._split_class_operand(), B, device)
        assert torch.isfinite(corr).all() and torch.isfinite(invn).all()
        s64 = torch.relu(corr.double()).pow(2).sum(dim=1)
        want = (1.0 / (torch.sqrt(s64.float()) + 1e-6))
        assert float(((invn - want).abs() / want).max()) < 5e-7              # fp32 group sums of 4, one rounding of s, sqrt, add, divide
        for picks in ([B - 1], [3, 0], list(range(B - 1, -1, -2))):
            sub = creator.create_os2d_head([cls[i] for i in picks])
            c2, i2 = _packed_corr(lib, fm, sub._split_class_operand(), len(picks), device)
            assert torch.equal(c2, corr[picks]) and torch.equal(i2, invn[picks])
        again = _packed_corr(lib, fm, head._split_class_operand(), B, device)
        assert torch.equal(again[0], corr) and torch.equal(again[1], invn)
        # the padded form (one 256-row tile per class) and whatever the head would pick: the same bits
        for form in (0, 4, 5, -1):          # padded, the same without half tiles at the tail, packed without them, the head's choice
            other = _packed_corr(lib, fm, head._split_class_operand(), B, device, form=form)
            assert torch.equal(other[0], corr) and torch.equal(other[1], invn), form


def test_dump_variant_builds_and_runs(device, tmp_path):
    """the -DOS2D_DIAG_DUMP build (tools/diag_pyramid_dump.py needs it) dead-locked in its first head forward -
    ``dumps_active()`` called itself under a non-recursive mutex.  Build the variant, register a dump slot, run one forward in
    a child process (a hang is a timeout, not a stuck test session) and look at the dumped correlation tensor."""
    import os
    import subprocess
    import sys
    repo = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    built = subprocess.run([sys.executable, "-m", "os2d_amd.build", "--variant", "dump_test", "-DOS2D_DIAG_DUMP"], cwd=repo,
                           capture_output=True, text=True, timeout=900)
    assert built.returncode == 0, built.stderr[-2000:]
    lib = built.stdout.strip().splitlines()[-1]
    script = r'''
import ctypes, sys, torch
sys.path.insert(0, "{repo}"); sys.path.insert(0, "{repo}/tests")
import util
from os2d_amd import _lib
from os2d_amd.utils import synthetic
lib = _lib.load(); dev = torch.device("cuda:0")
state = synthetic.make_transform_net_state(6, seed=1)
fm = synthetic.make_feature_map(32, 9, 11, seed=3).to(dev)
creator = util.make_head_creator(6, True, state, dev)
with torch.no_grad():
    head = creator.create_os2d_head([c.to(dev) for c in synthetic.make_class_feature_maps(8, 32, seed=5)])
    corr = torch.zeros(8 * 225 * 99, dtype=torch.float32, device=dev)
    lib.os2d_debug_set_dump(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), 0, _lib.ptr(corr), corr.numel() * 4)
    out = head(fm, precision="fftx3!")
    torch.cuda.synchronize()
    lib.os2d_debug_set_dump(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), 0, None, 0)
    again = head(fm, precision="fftx3!")
    torch.cuda.synchronize()
assert float(corr.abs().max()) > 0 and torch.isfinite(corr).all(), "nothing was dumped"
assert torch.equal(out[1], again[1])
print("DUMP_OK", float(corr.abs().max()))
'''.format(repo=repo)
    run = subprocess.run([sys.executable, "-c", script], cwd=repo, env=dict(os.environ, OS2D_HIP_LIB=lib), capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0 and "DUMP_OK" in run.stdout, (run.stdout[-1500:], run.stderr[-1500:])
