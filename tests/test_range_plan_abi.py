"""CPU: the host side of os2d_train_range_plan (os2d_amd/csrc_train/range_plan.hip, libos2d_train.so): the sizes of its two
result buffers and every argument check that fires before any launch, as (arguments, return code, os2d_train_last_error()) -
in the order of the checks."""
import ctypes

import pytest

import range_plan_model as RP

_OK, _ODD = 0x10000, 0x10004      # a non-null address nobody dereferences (256-byte aligned) and one that is only 4-byte aligned
NAMES = ("P w1 b1 bn1_weight bn1_bias bn1_running_mean bn1_running_var bn1_eps w2 b2 bn2_weight bn2_bias bn2_running_mean "
         "bn2_running_var bn2_eps w3 exps bounds stream").split()
POINTERS = [n for n in NAMES if n not in ("P", "bn1_eps", "bn2_eps", "stream")]
REQUIRED = ("w1", "b1", "w2", "b2", "w3", "exps", "bounds")
NULL = "os2d_train_range_plan: null pointer"
BN = "os2d_train_range_plan: BatchNorm of layer {} needs all four of weight/bias/running_mean/running_var"


@pytest.fixture(scope="module")
def lib():
    from os2d_amd import _train_lib, build
    build.build(verbose=False)
    return _train_lib.load()


def _args(**over):
    a = dict.fromkeys(POINTERS, _OK)
    a.update(P=6, bn1_eps=1e-5, bn2_eps=1e-5, stream=None)
    assert set(over) <= set(NAMES)
    a.update(over)
    return tuple(a[n] for n in NAMES)


def _refusals():
    rows = [(_args(**{name: None}), -1, NULL) for name in REQUIRED]
    rows += [
        (_args(w3=None, P=5), -1, NULL),                                                                     # 2x: pointers before P
        (_args(P=5), -1, "os2d_train_range_plan: bad P 5 (6 or 4)"),
        (_args(P=0, bn1_bias=None), -1, "os2d_train_range_plan: bad P 0 (6 or 4)"),                              # 2x: P before BatchNorm
    ]
    for layer in (1, 2):
        bn = ["bn{}_{}".format(layer, k) for k in ("weight", "bias", "running_mean", "running_var")]
        rows += [(_args(**{name: None}), -1, BN.format(layer)) for name in bn]                               # three of four
        rows.append((_args(**{name: None for name in bn[1:]}), -1, BN.format(layer)))                         # one of four
    rows += [
        (_args(bn1_weight=None, bn2_weight=None), -1, BN.format(1)),                                         # 2x: layer 1 first
        (_args(bn2_bias=None, bounds=_ODD), -1, BN.format(2)),                                               # 2x: BatchNorm before alignment
        (_args(bounds=_ODD), -1, "os2d_train_range_plan: bounds must be 8-byte, exps 4-byte aligned"),
        (_args(exps=0x10002), -1, "os2d_train_range_plan: bounds must be 8-byte, exps 4-byte aligned"),
    ]
    return rows


def test_buffer_sizes_are_the_documented_layout(lib):
    assert lib.os2d_train_range_plan_ints() == RP.INTS == 520 and lib.os2d_train_range_plan_doubles() == RP.DOUBLES == 192


def test_refusals_keep_their_code_text_and_order(lib):
    table = _refusals()
    assert len(table) >= 20
    for args, rc, text in table:
        lib.os2d_train_params_backward(_OK, 4, 5, 9, 13, _OK, None, None)          # another text: the row's call must set its own
        got = lib.os2d_train_range_plan(*args)
        assert (got, lib.os2d_train_last_error().decode()) == (rc, text), args
