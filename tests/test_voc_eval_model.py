"""CPU: tests/voc_eval_model.py (the VOC metric restated in vectorised torch, in the parallel formulation of the HIP kernels)
reproduces every fixture recorded from the reference: match, n_pos, tp, fp, prec, rec exactly, AP and the scalars within
1e-10.  The model is then the comparator for the shape too large to record (tests/test_voc_eval_gpu.py)."""
import numpy as np
import pytest
import torch

import voc_eval_cases as VC
import voc_eval_model as M
import voc_eval_util as U


@pytest.mark.parametrize("use_07", (False, True))
@pytest.mark.parametrize("thr", VC.THRESHOLDS)
@pytest.mark.parametrize("name", VC.CASES)
def test_model_reproduces_the_reference(name, thr, use_07):
    fx = U.fixture(name)
    images, preds, gts = U.resized_case(name)
    U.check_inputs(name, images, fx)
    p = U.model_pack(preds, gts, torch.device("cpu"))
    r = M.evaluate(p, VC.NUM_LABELS[name], thr, use_07)
    U.compare(fx, thr, use_07, U.model_bundle(p, r))


def test_small_case_covers_the_edge_cases():
    fx = U.fixture("small")
    assert fx["prec_len_t50"][1] == 0 and fx["rec_len_t50"][1] == 0          # ground truth, no detection: empty curves
    assert fx["prec_len_t50"][2] > 0 and fx["rec_len_t50"][2] == -1          # detections, no ground truth: rec is None
    assert fx["n_pos"][3] == 0 and (fx["match_t50"] == -1).any()             # a class of difficult boxes only
    assert np.isnan(fx["ap_t50"][2]) and np.isnan(fx["ap_t50"][3]) and fx["ap_t50"][1] == 0.0
    assert not np.array_equal(fx["match_t50"], fx["match_t75"])


def test_ties_keep_increasing_index():
    """Equal scores: descending score, then increasing packed index - the first of two equal detections on one box wins."""
    box = torch.tensor([[10., 10., 50., 50.]])
    p = M.pack([box.repeat(2, 1), box], [torch.tensor([0.5, 0.5]), torch.tensor([0.5])], [torch.zeros(2), torch.zeros(1)],
               [box, box], [torch.zeros(1), torch.zeros(1)], [torch.zeros(1), torch.zeros(1)], torch.device("cpu"))
    r = M.evaluate(p, 1, 0.5)
    assert r["match"].tolist() == [1, 0, 1] and r["order_joint"].tolist() == [0, 1, 2]
