"""GPU: the order-independent d corr scatter of the decode backward (os2d_train_decode_backward_det, include/os2d_train.h) and
the ``deterministic`` switch of the head: accuracy against the float64 model, the integers adding exactly, independence of the
order and the company of a pair, repeatability, the NaN policy, null upstream gradients, and every gradient of the head bit for
bit through autograd.  (The rule, the refusals and the kernels' resources: tests/test_backward_det.py.)"""
import functools
import itertools

import pytest
import torch

import backward_det_model as D
import backward_model as M
import test_backward_stages_gpu as S
import test_head_backward_gpu as HB
import util
from test_backward_stages_gpu import PIN, bits, dev, nan

pytestmark = pytest.mark.gpu


def run_det(device, inp, P, inverse, stride, rec_field, use=(True, True, True), zeros_for_absent=False):
    """os2d_train_decode_backward_det on NaN-filled dparams, the prefill pattern in dcorr and a workspace of 0xFF bytes.
    Returns (dcorr, dparams, the int64 sums [NB,225,HW], the pair words [NB]) on the CPU."""
    lib = S._lib()
    NB, _, H, W = inp["corr"].shape
    ups = []
    for name, on in zip(("dcls", "dcls_det", "dloc"), use):
        ups.append(dev(inp[name], device) if on else dev(torch.zeros_like(inp[name]), device) if zeros_for_absent else None)
    corr, params = dev(inp["corr"], device), dev(inp["params"], device)
    dcorr = dev(inp["prefill"], device)
    dparams = nan(device, NB, P, H * W)
    nbytes = int(lib.os2d_train_decode_backward_det_workspace_bytes(NB, H, W))
    assert nbytes == D.workspace_bytes(NB, H, W)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
    S._check(lib.os2d_train_decode_backward_det(S._ptr(corr), S._ptr(params), S._ptr(ups[0]), S._ptr(ups[1]), S._ptr(ups[2]), NB, H, W, P,
                                                1 if inverse else 0, stride, rec_field, S._ptr(dcorr), S._ptr(dparams), S._ptr(ws), nbytes,
                                                S._stream(device)), "decode_backward_det")
    raw = ws.cpu()
    n_acc = NB * M.K * H * W * 8
    acc = raw[:n_acc].view(torch.int64).view(NB, M.K, H * W)
    words = raw[n_acc:n_acc + 4 * NB].view(torch.int32)
    return dcorr.cpu(), dparams.cpu(), acc, words


def select(inp, pairs):
    """The inputs of some pairs of a case, in the order given."""
    idx = torch.tensor(pairs)
    return {k: v[idx].clone() for k, v in inp.items()}


# ---------------------------------------------------------------------------------------------------------- accuracy
def _check_accuracy(device, tag, inp, dcorr_ref, P, inverse, stride, rec_field):
    dcorr, dparams, acc, words = run_det(device, inp, P, inverse, stride, rec_field)
    assert bool(torch.isfinite(dcorr).all()) and bool(torch.isfinite(dparams).all())
    err = M.rel_err(dcorr, inp["prefill"].double() + dcorr_ref)
    S.report("decode_dcorr det", tag, err)
    assert err < PIN["decode_dcorr"]
    _, dparams_float = S.run_decode(device, inp, P, inverse, stride, rec_field)
    assert torch.equal(bits(dparams), bits(dparams_float)), "dparams is the same code on both routes"
    g = inp["dcls"].float() + inp["dcls_det"].float()
    assert words.tolist() == [D.float_bits(float(g[nb].abs().max())) for nb in range(g.size(0))]
    assert int(acc.abs().max()) < 2 ** 56


@pytest.mark.parametrize("name", sorted(M.DECODE_CASES))
def test_decode_backward_det(device, name):
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    inp, dcorr_ref, _ = D.case_reference(name)
    _check_accuracy(device, name, inp, dcorr_ref, P, inverse, stride, rec_field)


@pytest.mark.parametrize("inverse", [True, False], ids=["inv", "fwd"])
def test_decode_backward_det_hand_placed_locations(device, inverse):
    inp, dcorr_ref, _ = D.hand_reference(inverse)
    _check_accuracy(device, "hand inverse={}".format(inverse), inp, dcorr_ref, 6, inverse, 16, 16)


# ---------------------------------------------------------------------------------------------------------- integers add exactly
def test_sums_of_two_sets_of_locations_add_as_integers(device):
    """Each set holds a location with |dcls + dcls_det| = 1 exactly and nothing larger: the three runs share one exponent, and
    the sums of the union are the sums of the parts, cell by cell."""
    name = "17x19_p6_inv_s16"
    P, inverse, stride, rec_field, NB, H, W, _ = M.DECODE_CASES[name]
    inp = {k: v.clone() for k, v in D.case_reference(name)[0].items()}
    g = inp["dcls"] + inp["dcls_det"]
    inp["dcls"] = g / (2 * g.abs().max())                 # every |value| <= 0.5
    inp["dcls_det"] = torch.zeros_like(g)
    first = (torch.arange(H * W) % 2 == 0).view(1, H, W)  # set 1: the even locations
    inp["dcls"].view(NB, -1)[:, 0] = 1.0                  # a member of set 1
    inp["dcls"].view(NB, -1)[:, H * W - 2] = -1.0         # a member of set 2 (H W - 2 = 321 is odd)
    assert bool(first.view(-1)[0]) and not bool(first.view(-1)[H * W - 2])
    accs = []
    for mask in (first, ~first, torch.ones_like(first)):
        part = dict(inp, dcls=inp["dcls"] * mask)
        _, _, acc, words = run_det(device, part, P, inverse, stride, rec_field)
        assert words.tolist() == [0x3F800000] * NB
        accs.append(acc)
    assert int(accs[0].abs().max()) > 0 and int(accs[1].abs().max()) > 0
    assert int(((accs[0] != 0) & (accs[1] != 0)).sum()) > 0, "the two sets share cells"
    assert torch.equal(accs[2], accs[0] + accs[1])


def test_scatter_rounds_exactly_known_addends_to_the_nearest_integer(device):
    """Every location of a 3x3 map samples with all 121 points clamped to x = W - 1, y = 0 (HAND_THETA[4]): the bilinear
    weights are exactly 1 and 0, so channel ch's cell (0, 2) receives, per location, the one addend fp32(g * fp32(1/121)) - known
    bit for bit on the CPU.  Location 0 has g = 1 (e = 54); the others are 2^-26 .. 2^-40 small, so their scaled addends have
    fractional parts: the sums the kernel leaves must be the sums of their nearest integers, exactly."""
    import numpy as np
    H = W = 3
    th = torch.tensor(M.HAND_THETA[4]).reshape(6)
    g = torch.Generator().manual_seed(5)
    small = (1 + torch.rand(8, generator=g)) * 2.0 ** -torch.tensor([26.0, 28, 30, 31, 33, 35, 38, 40])
    small[1::2] *= -1
    grads = torch.cat([torch.ones(1), small]).float()
    inp = dict(corr=0.3 * torch.randn(1, M.K, H, W, generator=g), params=th.view(1, 6, 1, 1).expand(1, 6, H, W).contiguous(),
               dcls=grads.view(1, H, W), dcls_det=torch.zeros(1, H, W), dloc=torch.zeros(1, 4, H, W), prefill=torch.zeros(1, M.K, H * W))
    _, _, acc, words = run_det(device, inp, 6, False, 16, 16)
    e = D.exponent(int(words[0]), H, W)
    assert int(words[0]) == 0x3F800000 and e == 54
    addends = (grads.numpy() * (np.float32(1.0) / np.float32(121.0))).astype(np.float32).astype(np.float64) * 2.0 ** e
    assert int((addends != np.floor(addends)).sum()) >= 6, "the small addends fall between grid points"
    nearest, floor = int(np.rint(addends).astype(np.int64).sum()), int(np.floor(addends).astype(np.int64).sum())
    assert nearest != floor
    lo, hi = M.O.POOL_BORDER, M.T - M.O.POOL_BORDER
    pooled = torch.zeros(M.T, M.T, dtype=torch.bool)
    pooled[lo:hi, lo:hi] = True                               # symmetric in (i, j): the channel order does not matter
    expected = torch.zeros(M.K, H * W, dtype=torch.int64)
    expected[pooled.view(-1), 0 * W + (W - 1)] = nearest
    assert torch.equal(acc[0], expected)


# ---------------------------------------------------------------------------------------------------------- order, company, repeat
def test_pairs_do_not_depend_on_their_order_or_their_company(device):
    name = "17x19_p6_inv_s16"
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    inp = D.case_reference(name)[0]
    dcorr, dparams, _, _ = run_det(device, inp, P, inverse, stride, rec_field)
    perm = [2, 0, 1]
    dcorr_p, dparams_p, _, _ = run_det(device, select(inp, perm), P, inverse, stride, rec_field)
    for k, nb in enumerate(perm):
        assert torch.equal(bits(dcorr_p[k]), bits(dcorr[nb])) and torch.equal(bits(dparams_p[k]), bits(dparams[nb])), nb
    dcorr_1, dparams_1, _, _ = run_det(device, select(inp, [1]), P, inverse, stride, rec_field)
    assert torch.equal(bits(dcorr_1[0]), bits(dcorr[1])) and torch.equal(bits(dparams_1[0]), bits(dparams[1]))


@pytest.mark.parametrize("case", ["38x38_p6_inv_s16", "hand_inv"])
def test_three_calls_give_the_same_bits(device, case):
    if case == "hand_inv":
        inp, (P, inverse, stride, rec_field) = D.hand_reference(True)[0], (6, True, 16, 16)
    else:
        inp, (P, inverse, stride, rec_field) = D.case_reference(case)[0], M.DECODE_CASES[case][:4]
    runs = [run_det(device, inp, P, inverse, stride, rec_field) for _ in range(3)]
    for dcorr, dparams, acc, _ in runs[1:]:
        assert torch.equal(bits(dcorr), bits(runs[0][0])) and torch.equal(bits(dparams), bits(runs[0][1]))
        assert torch.equal(acc, runs[0][2])


# ---------------------------------------------------------------------------------------------------------- NaN policy, zeros
def test_a_nan_marks_its_pair_and_a_pair_without_gradient_keeps_its_prefill(device):
    name = "9x13_p6_inv_s16"
    P, inverse, stride, rec_field, NB, H, W, _ = M.DECODE_CASES[name]
    clean = {k: v.clone() for k, v in D.case_reference(name)[0].items()}
    clean["dcls"][0] = 0                                   # pair 0: no upstream class gradient at all
    clean["dcls_det"][0] = 0
    dcorr, dparams, acc, words = run_det(device, clean, P, inverse, stride, rec_field)
    assert words[0] == 0 and int(acc[0].abs().max()) == 0
    assert torch.equal(bits(dcorr[0]), bits(clean["prefill"][0])), "a pair with zero gradients leaves its prefill bits"
    assert bool(torch.isfinite(dcorr).all()) and not torch.equal(bits(dcorr[1]), bits(clean["prefill"][1]))
    dirty = {k: v.clone() for k, v in clean.items()}
    dirty["dcls"][1, H // 2, W // 2] = float("nan")
    dcorr_n, dparams_n, _, words_n = run_det(device, dirty, P, inverse, stride, rec_field)
    assert int(words_n[1]) >= 0x7F800000
    assert bool(torch.isnan(dcorr_n[1]).all()), "every cell of the pair"
    for nb in (0, 2):
        assert torch.equal(bits(dcorr_n[nb]), bits(dcorr[nb])) and torch.equal(bits(dparams_n[nb]), bits(dparams[nb])), nb


@pytest.mark.parametrize("name", ["9x13_p6_inv_s16", "9x13_p4_fwd_s16"])
def test_null_upstream_gradients_equal_explicit_zeros(device, name):
    """The eight subsets of tests/test_backward_stages_gpu.py::test_decode_backward_null_upstream_gradients: an equality here."""
    P, inverse, stride, rec_field = M.DECODE_CASES[name][:4]
    inp = D.case_reference(name)[0]
    for use in itertools.product((True, False), repeat=3):
        dcorr, dparams, _, _ = run_det(device, inp, P, inverse, stride, rec_field, use=use)
        assert bool(torch.isfinite(dparams).all()) and bool(torch.isfinite(dcorr).all())
        if not any(use):
            assert torch.count_nonzero(dparams) == 0
            assert torch.equal(bits(dcorr), bits(inp["prefill"]))
            continue
        dcorr0, dparams0, _, _ = run_det(device, inp, P, inverse, stride, rec_field, use=use, zeros_for_absent=True)
        assert torch.equal(bits(dparams), bits(dparams0)), use
        assert torch.equal(bits(dcorr), bits(dcorr0)), use
        if not (use[0] or use[1]):
            assert torch.equal(bits(dcorr), bits(inp["prefill"]))


# ---------------------------------------------------------------------------------------------------------- through autograd
AUTOGRAD_CASES = ["v2_affine_inverse", "simple_affine_p4", "odd_c67_9x13"]


@functools.lru_cache(maxsize=None)
def _autograd_reference(name):
    from os2d_amd.utils import synthetic
    P, inverse, A, C, H, W, sizes, B = HB.CASES[name]
    state = synthetic.make_transform_net_state(P, seed=3)
    fm = synthetic.make_feature_map(C, H, W, seed=5, A=A)
    class_fms = synthetic.make_class_feature_maps(B, C, sizes=sizes, seed=400)
    ups = HB.upstream(A, B, H, W, 7)
    return state, fm, class_fms, ups, HB.oracle_grads(fm, class_fms, state, inverse, *ups)


def _flat(grads):
    out = {"fm": grads["fm"]}
    out.update({"class{}".format(b): g for b, g in enumerate(grads["class"])})
    out.update({k: grads[k] for k in HB.PARAM_KEYS})
    return out


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name", AUTOGRAD_CASES)
def test_every_gradient_of_the_head_is_bit_reproducible(device, monkeypatch, name, precision):
    """Two independent forward + backward passes on fresh tensors: the same bits for the image map, every raw class map and the
    ten TransformNet tensors; each within the end-to-end tolerance of the CPU oracle."""
    P, inverse = HB.CASES[name][:2]
    state, fm, class_fms, ups, ref = _autograd_reference(name)
    monkeypatch.setenv("OS2D_TRAIN_PRECISION", precision)        # HB.hip_grads builds its own creator: it follows the environment
    monkeypatch.setenv("OS2D_DETERMINISTIC", "1")
    from os2d_amd import _train_lib
    runs = []
    for _ in range(2):
        spy = _Spy(_train_lib.load())
        with monkeypatch.context() as m:
            m.setattr(_train_lib, "load", lambda: spy)
            got, _, creator = HB.hip_grads(device, fm, class_fms, state, P, inverse, *ups)
        assert creator.deterministic is None
        assert spy.calls.count("os2d_train_decode_backward_det") == 1 and "os2d_train_decode_backward" not in spy.calls
        assert ("os2d_train_corr_backward_ex" in spy.calls) and len(spy.calls) > 10, "the whole backward went through the spy"
        runs.append(_flat(got))
    ref = _flat(ref)
    assert sorted(runs[0]) == sorted(ref) and len(ref) == 1 + len(class_fms) + 10
    errs = {k: HB.rel_err(runs[0][k], ref[k]) for k in ref}
    print(name, precision, "deterministic, relative max errors:", {k: "{:.2e}".format(v) for k, v in errs.items()})
    assert not {k: v for k, v in errs.items() if not v < HB.TOL}, errs
    differing = [k for k in ref if not torch.equal(bits(runs[0][k]), bits(runs[1][k]))]
    assert not differing, differing


# ---------------------------------------------------------------------------------------------------------- the switch
def _head(device, deterministic=None):
    state, fm, class_fms, _ = HB._small(device)
    creator = util.make_head_creator(6, True, state, device)
    assert creator.deterministic is None
    creator.deterministic = deterministic
    head = creator.create_os2d_head([c.to(device).requires_grad_(True) for c in class_fms])
    return creator, head, fm.to(device).requires_grad_(True)


class _Spy:
    """Stands in for the loaded library: records the names of the entry points that are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def _spied_backward(monkeypatch, head, fm):
    from os2d_amd import _train_lib
    spy = _Spy(_train_lib.load())
    out = head(fm)
    with monkeypatch.context() as m:
        m.setattr(_train_lib, "load", lambda: spy)
        (out[0].sum() + out[1].sum() + out[2].sum()).backward()
    return out, spy.calls


def test_switch_is_copied_recorded_and_selects_the_entry_point(device, monkeypatch):
    monkeypatch.delenv("OS2D_DETERMINISTIC", raising=False)
    assert not torch.are_deterministic_algorithms_enabled()
    creator, head, fm = _head(device, True)
    assert head.deterministic is True and head.last_deterministic is None
    out_on, calls = _spied_backward(monkeypatch, head, fm)
    assert head.last_deterministic is True
    assert "os2d_train_decode_backward_det" in calls and "os2d_train_decode_backward" not in calls
    assert "os2d_train_decode_backward_det_workspace_bytes" in calls
    creator, head_off, fm_off = _head(device, None)
    assert head_off.deterministic is None
    out_off, calls = _spied_backward(monkeypatch, head_off, fm_off)
    assert head_off.last_deterministic is False
    assert "os2d_train_decode_backward" in calls and not [c for c in calls if "_det" in c]
    for a, b in zip(out_on, out_off):
        assert torch.equal(bits(a), bits(b)), "the forward does not change"
    assert fm.grad is not None and fm_off.grad is not None
    assert float((fm.grad - fm_off.grad).abs().max()) < HB.TOL * float(fm_off.grad.abs().max())


def test_environment_and_torch_flag_turn_it_on_and_an_explicit_false_wins(device, monkeypatch):
    monkeypatch.setenv("OS2D_DETERMINISTIC", "1")
    _, head, fm = _head(device, None)
    head(fm)
    assert head.last_deterministic is True
    head.deterministic = False
    head(fm)
    assert head.last_deterministic is False
    monkeypatch.setenv("OS2D_DETERMINISTIC", "0")
    head.deterministic = None
    head(fm)
    assert head.last_deterministic is False
    monkeypatch.delenv("OS2D_DETERMINISTIC")
    torch.use_deterministic_algorithms(True)
    try:
        head(fm)
        assert head.last_deterministic is True
        _, calls = _spied_backward(monkeypatch, head, fm)
        assert "os2d_train_decode_backward_det" in calls
        head.deterministic = False
        head(fm)
        assert head.last_deterministic is False
        creator, head2, fm2 = _head(device, False)
        _, calls = _spied_backward(monkeypatch, head2, fm2)
        assert head2.last_deterministic is False and not [c for c in calls if "_det" in c]
    finally:
        torch.use_deterministic_algorithms(False)


def test_a_switch_that_is_no_bool_raises(device, monkeypatch):
    monkeypatch.delenv("OS2D_DETERMINISTIC", raising=False)
    _, head, fm = _head(device, "on")
    with pytest.raises(ValueError, match="deterministic"):
        head(fm)
    with torch.no_grad():
        head(fm)                                          # the inference route does not look at it
