"""tests/soft_nms_ref.py - the fp32 model of detect.hip's Soft-NMS pass - against hand-computed cases and detect_ref's hard NMS, the
properties of the GPU tests' inputs, and dsl_amd.sweep._test_cfg's reading of test_cfg.nms."""
import itertools
import types

import numpy as np
import pytest
import torch

import detect_ref as R
import soft_nms_ref as S

F = np.float32


def boxes(*rows):
    return np.array(rows, F)


def run(b, lab, sc, method, iou_thr=0.3, max_per_img=100, **kw):
    d, l, _ = S.soft_nms(boxes(*b), np.array(lab), np.array(sc, F), iou_thr, max_per_img, method, **kw)
    return d[:, 4].numpy().astype(np.float64), l.tolist(), d[:, :4].tolist()


def test_linear_by_hand():
    """Class 0: A [0,0,10,10] 0.9, B [0,0,10,5] 0.8, C [20,20,30,30] 0.7.  All labels 0: the class offset is 0.
    Pick A (0.9).  IoU(A, B) = 50 / (100 + 50 - 50) = 0.5 > 0.3: B -> 0.8 * (1 - 0.5) = 0.4.  IoU(A, C) = 0: C stays 0.7.
    Pick C (0.7); IoU(C, B) = 0.  Pick B (0.4).  Output order A, C, B."""
    s, l, b = run([[0, 0, 10, 10], [0, 0, 10, 5], [20, 20, 30, 30]], [0, 0, 0], [0.9, 0.8, 0.7], 'linear')
    assert b == [[0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 5]]
    assert s == pytest.approx([0.9, 0.7, 0.4], rel=1e-6)


def test_gaussian_by_hand_with_a_box_that_disappears():
    """sigma 0.5, min_score 0.05.  A [0,0,10,10] 0.9, B [0,0,10,8] 0.5, C [0,0,10,10] 0.6 (A's twin).
    Pick A.  IoU(A, B) = 0.8: B -> 0.5 * exp(-0.64 / 0.5) = 0.5 * 0.278037 = 0.139019.  IoU(A, C) = 1: C -> 0.6 * exp(-2) = 0.081201.
    Pick B (0.139019).  IoU(B, C) = 0.8: C -> 0.081201 * 0.278037 = 0.022577 < 0.05: C is dropped.  Output A, B."""
    s, l, b = run([[0, 0, 10, 10], [0, 0, 10, 8], [0, 0, 10, 10]], [0, 0, 0], [0.9, 0.5, 0.6], 'gaussian', min_score=0.05)
    assert b == [[0, 0, 10, 10], [0, 0, 10, 8]]
    assert s == pytest.approx([0.9, 0.5 * np.exp(-1.28)], rel=1e-6)
    # with the default min_score C stays and comes out last
    s, l, b = run([[0, 0, 10, 10], [0, 0, 10, 8], [0, 0, 10, 10]], [0, 0, 0], [0.9, 0.5, 0.6], 'gaussian')
    assert s == pytest.approx([0.9, 0.5 * np.exp(-1.28), 0.6 * np.exp(-2.0) * np.exp(-1.28)], rel=1e-6)


def test_naive_by_hand_and_classes_do_not_interact():
    """The same two boxes in class 0 and class 1: A [0,0,10,10], B [0,0,10,5] (IoU 0.5 > 0.3), scores class 0: 0.9, 0.8; class 1:
    0.85, 0.6.  The class offset is label * (10 + 1).  Per class, A is picked and B's score becomes 0 < min_score: dropped.  Were the
    classes one, class 1's A (IoU 1 with class 0's A) would be dropped as well.  Output: A of class 0 (0.9), A of class 1 (0.85)."""
    s, l, b = run([[0, 0, 10, 10], [0, 0, 10, 5], [0, 0, 10, 10], [0, 0, 10, 5]], [0, 0, 1, 1], [0.9, 0.8, 0.85, 0.6], 'naive')
    assert l == [0, 1] and b == [[0, 0, 10, 10], [0, 0, 10, 10]]
    assert s == pytest.approx([0.9, 0.85], rel=1e-7)


def test_equal_scores_go_to_the_lower_candidate_number():
    s, l, b = run([[0, 0, 10, 10], [20, 0, 30, 10], [40, 0, 50, 10]], [0, 0, 0], [0.5, 0.7, 0.7], 'linear')
    assert b == [[20, 0, 30, 10], [40, 0, 50, 10], [0, 0, 10, 10]]


CASES = [(lv, C) for lv in (1, 2, 'long') for C in (3, 80)]


@pytest.mark.parametrize('levels,C', CASES)
def test_naive_keeps_what_the_hard_nms_keeps(levels, C):
    """Same threshold, min_score so small that nothing but a suppressed box (score 0) is dropped."""
    for thr in (0.3, 0.7, 0.85):
        case = S.case(levels, C, 100, iou_thr=thr)
        for (d, l, _), (hd, hl, _) in zip(S.detect(case, 'naive', min_score=1e-30), R.detect(case)):
            assert len(d) == len(hd) >= 2
            assert torch.equal(l, hl) and torch.equal(d.float(), hd)


@pytest.mark.parametrize('levels,C', CASES)
def test_competing_scores_are_far_apart(levels, C):
    """The property the GPU tests rest on: at every pick the two highest current scores of the class, and any two adjacent scores of
    the pooled output, differ by more than 100 x the score tolerance of the leg - so a device within the tolerance makes every
    choice as the model does.  Also what the inputs were built to hold: a long chain, a class of one, an empty class."""
    for method, ms in itertools.product(('linear', 'gaussian', 'naive'), (S.LONG_MIN_SCORE, 1e-3)):
        tol = S.score_rtol(S.cluster_size(levels) - 1, method)
        case = S.case(levels, C, 100)
        for i, (d, l, rec) in enumerate(S.detect(case, method, min_score=ms, bound=False)):
            assert S.min_gap(rec) > 100 * tol, (method, ms, i, S.min_gap(rec), tol)
            assert rec['n_decays'] <= S.cluster_size(levels) - 1
            counts = np.bincount(S.valid_pairs(*R.candidates(case, i), case.score_thr)[1], minlength=C)
            assert counts.max() == S.cluster_size(levels) and (counts == 1).sum() >= 1 and (counts == 0).sum() >= 1
            if method != 'naive' and ms == S.LONG_MIN_SCORE and levels != 'long':
                assert rec['n_decays'] == S.cluster_size(levels) - 1          # the whole cluster comes out, one after the other


def test_aug_inputs_have_the_margin_too():
    views, metas = S.aug_views()
    for method in ('linear', 'gaussian'):
        d, l, rec = S.aug(views, metas, 1000, 0.05, 0.3, 100, method, min_score=S.LONG_MIN_SCORE)
        assert S.min_gap(rec) > 100 * S.score_rtol(S.AUG_CLUSTER - 1, method)
        assert rec['n_decays'] == S.AUG_CLUSTER - 1


@pytest.mark.parametrize('levels,C', [(2, 3), (1, 80), ('long', 80)])
def test_stopping_a_class_after_max_per_img_picks_is_exact(levels, C):
    for method in ('linear', 'gaussian'):
        case = S.case(levels, C, 5)
        for a, b in zip(S.detect(case, method, min_score=S.LONG_MIN_SCORE, bound=True), S.detect(case, method, min_score=S.LONG_MIN_SCORE, bound=False)):
            assert len(a[0]) == 5 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert len(b[2]['emitted']) > 5 * 4


def test_exact_inputs():
    assert all(len(d) == 0 for d, _, _ in S.detect(S.exact_case('empty'), 'linear'))
    for method in S.METHODS:
        for d, l, rec in S.detect(S.exact_case('drop'), method, min_score=0.45):
            assert d[:, 4].tolist() == [1.0] and rec['n_decays'] == 0


def test_exp_error_is_the_recorded_one():
    """soft_nms_ref.EXP_ERR: the model's fp32 exp against the fp64 exp of the same arguments, over every gaussian decay of the inputs."""
    args = []
    for levels, C in CASES:
        for _, _, rec in S.detect(S.case(levels, C, 100), 'gaussian', min_score=S.LONG_MIN_SCORE, bound=False):
            args += rec['exp_args']
    args += S.aug(*S.aug_views(), 1000, 0.05, 0.3, 100, 'gaussian', min_score=S.LONG_MIN_SCORE)[2]['exp_args']
    err = S.exp_error(args)
    print('exp: max relative error', err, 'over', sum(len(a) for a in args), 'arguments')
    assert 0 < err <= S.EXP_ERR


# ---- test_cfg ---------------------------------------------------------------------------------------------------------------------
def cfg_of(**test_cfg):
    from dsl_amd.sweep import _test_cfg
    return _test_cfg(types.SimpleNamespace(test_cfg=test_cfg))


def test_cfg_hard_nms_is_unchanged():
    from dsl_amd import _lib as L
    hard = dict(nms_method=L.NMS_HARD, soft_sigma=0.0, soft_min_score=0.0)
    assert cfg_of() == dict(nms_pre=1000, max_per_img=100, score_thr=0.05, iou_thr=0.5, **hard)
    assert cfg_of(nms=dict(type='nms', iou_threshold=0.6), nms_pre=500, max_per_img=50, score_thr=0.1) == dict(
        nms_pre=500, max_per_img=50, score_thr=0.1, iou_thr=0.6, **hard)
    assert cfg_of(nms=dict(iou_thr=0.45))['iou_thr'] == 0.45 and cfg_of(nms=dict(type='nms'))['iou_thr'] == 0.5


def test_cfg_soft_nms_defaults_and_every_key():
    from dsl_amd import _lib as L
    got = cfg_of(nms=dict(type='soft_nms'))
    assert got == dict(nms_pre=1000, max_per_img=100, score_thr=0.05, iou_thr=0.3, nms_method=L.NMS_LINEAR, soft_sigma=0.5, soft_min_score=1e-3)
    got = cfg_of(nms=dict(type='soft_nms', iou_threshold=0.4, method='gaussian', sigma=0.25, min_score=0.01), max_per_img=7)
    assert got == dict(nms_pre=1000, max_per_img=7, score_thr=0.05, iou_thr=0.4, nms_method=L.NMS_GAUSSIAN, soft_sigma=0.25, soft_min_score=0.01)
    assert cfg_of(nms=dict(type='soft_nms', method='naive'))['nms_method'] == L.NMS_NAIVE
    assert (L.NMS_HARD, L.NMS_LINEAR, L.NMS_GAUSSIAN, L.NMS_NAIVE) == (0, 1, 2, 3) and S.METHODS == dict(linear=1, gaussian=2, naive=3)
    with pytest.raises(ValueError, match='method'):
        cfg_of(nms=dict(type='soft_nms', method='quadratic'))


def test_cfg_unknown_type_is_refused():
    with pytest.raises(NotImplementedError, match="'nms' and 'soft_nms'"):
        cfg_of(nms=dict(type='nms_match', iou_threshold=0.5))


def test_descriptor_carries_the_fields_at_its_end():
    from dsl_amd import _lib as L
    names = [f[0] for f in L.DetDesc._fields_]
    assert names[-3:] == ['nms_method', 'soft_sigma', 'soft_min_score'] and names[-4] == 'ctr'
    assert L.DetDesc.nms_method.offset == L.DetDesc.ctr.offset + 8
