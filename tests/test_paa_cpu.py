"""PAA without a GPU: tests/paa_ref.py against what the reference's own PAAHead and sklearn's GaussianMixture computed
(tests/golden/paa_*.npz, written by tests/golden/make_paa_golden.py), and the configuration surface of PAAHead / PAA."""
import copy

import numpy as np
import pytest
import torch

import paa_ref as PR
from test_atss_cpu import atss_model_cfg
from util import levels_to_flat

T = torch.from_numpy
CASES = 'abcdefgnw'
BAD_SAMPLES = (32.241912841796875, 78.50801849365234)      # float32 values: test_ref_gmm_reports_a_non_positive_variance


def load_case(d):
    B, C = int(d['B']), int(d['num_classes'])
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    return dict(B=B, C=C, sizes=sizes, topk=int(d['topk']), anchor_scale=float(d['anchor_scale']), stds=tuple(float(v) for v in d['stds']),
                thr=float(d['pos_iou_thr']), bbox_weight=float(d['bbox_weight']), iou_weight=float(d['iou_weight']),
                cls_weight=float(d['cls_loss_weight']), pads=[tuple(int(v) for v in p) for p in d['pads']],
                gts=[T(d[f'gt{i}']) for i in range(B)], gls=[T(d[f'gl{i}']) for i in range(B)],
                cls=levels_to_flat([T(d[f'cls{l}']) for l in range(5)]), reg=levels_to_flat([T(d[f'reg{l}']) for l in range(5)]),
                iou=levels_to_flat([T(d[f'iou{l}']) for l in range(5)])[:, 0], scales=T(d['scales']))


def ref_assign(c):
    return PR.assign(c['sizes'], c['gts'], c['gls'], c['pads'], c['thr'], c['anchor_scale'], c['C'])


def ref_reassign(c, a, ploss):
    return PR.reassign(ploss, a, c['sizes'], c['B'], [len(g) for g in c['gts']], c['topk'], c['C'])


def ref_loss(c, a, re, cls, reg, iou, scales):
    return PR.loss(cls, reg, iou, scales, a, re, c['sizes'], c['B'], c['C'], c['anchor_scale'], c['stds'], c['bbox_weight'], c['cls_weight'],
                   c['iou_weight'])


def test_fixtures_cover_the_cases(golden):
    d = {k: golden(f'paa_{k}.npz') for k in CASES}
    assert all(str(v['sklearn']) == '1.7.2' for v in d.values()) and str(golden('paa_det_a.npz')['sklearn']) == '1.7.2'
    assert int(d['a']['num_classes']) == 80 and all(int(d[k]['num_classes']) == 20 for k in 'bcdegnw') and int(d['f']['num_classes']) == 18
    assert len(d['b']['gt1']) == 0 and len(d['b']['gt0']) > 0 and len(d['n']['gt0']) == 0 and len(d['n']['gt1']) == 0
    assert [int(v) for v in d['e']['pads'][1]] == [96, 128] and (int(d['f']['topk']), float(d['f']['anchor_scale']), float(d['f']['pos_iou_thr'])) == (3, 4.0, 0.2)
    # d: no anchor reaches pos_iou_thr for the small boxes - every candidate of theirs comes from the low-quality pass - and of the
    # two boxes whose tied anchors coincide the later one has them all
    assert int(d['d']['box_n'][1]) == 0 and int(d['d']['box_n'][2]) == 9 and int(d['d']['box_flag'][1]) == 1
    assert bool(((d['g']['box_n'] == 1) & (d['g']['box_flag'] == 1)).any())
    assert 4 <= len(d['w']['gt0']) + len(d['w']['gt1']) <= 6
    assert all(bool((d[k]['box_iter'][d[k]['box_flag'] == 0] >= 2).all()) for k in CASES)
    assert max(int(d[k]['box_iter'].max()) for k in 'abcdefgw') > 15      # long and short fits are both present


@pytest.mark.parametrize('case', CASES)
def test_ref_assignment_and_reassignment_equal_reference(golden, case):
    d = golden(f'paa_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    assert torch.equal(a['cand_gt'], T(d['cand_gt'])) and torch.equal(a['labels'], T(d['labels0']))
    assert torch.equal(a['targets'], T(d['targets'])) and torch.equal(a['cls_weight'], T(d['cls_weight']))
    pl = PR.pos_loss(c['cls'], c['reg'], c['scales'], a, c['sizes'], c['B'], c['C'], c['anchor_scale'], c['stds'], c['bbox_weight'], c['cls_weight'])
    assert torch.allclose(pl, T(d['pos_loss']).double(), rtol=1e-5, atol=0)
    re = ref_reassign(c, a, d['pos_loss'])
    assert len(re['boxes']) == len(d['box_n'])
    for r, b in enumerate(re['boxes']):
        n = int(d['box_n'][r])
        assert (b['image'], b['box']) == (int(d['box_image'][r]), int(d['box_box'][r]))
        assert np.array_equal(b['index'], d['box_index'][r, :n]) and np.array_equal(b['samples'], d['box_samples'][r, :n])      # the top-k sets
        assert b['flag'] == int(d['box_flag'][r]) and b['n_iter'] == int(d['box_iter'][r])
        if b['flag'] == 0:
            assert np.array_equal(b['pred'], d['box_pred'][r, :n])
            assert np.abs(b['scores'] - d['box_scores'][r, :n]).max() < 1e-6
            assert min(b['stop_margin'], b['pred_margin'], b['gap']) >= (1e-4 if case == 'w' else 1e-6) * 0.99
    assert torch.equal(re['labels'], T(d['labels'])) and re['npos'] == [int(v) for v in d['npos']]


@pytest.mark.parametrize('case', CASES)
def test_ref_losses_and_gradients_equal_reference(golden, case):
    d = golden(f'paa_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    re = ref_reassign(c, a, d['pos_loss'])
    x, r, t, s = (v.double().requires_grad_() for v in (c['cls'], c['reg'], c['iou'], c['scales']))
    lc, lb, li, it = ref_loss(c, a, re, x, r, t, s)
    (lc + lb + li).backward()
    for k, v in (('loss_cls', lc), ('loss_bbox', lb), ('loss_iou', li)):
        assert float(v.detach()) == pytest.approx(float(d[k]), rel=1e-5, abs=1e-7), k
    assert torch.allclose(it, T(d['iou_target']).double(), rtol=1e-5, atol=1e-6)
    if case == 'n':
        assert float(lb) == 0.0 and float(li) == 0.0 and float(r.grad.abs().max()) == 0.0      # max(num_pos, n) = 2 under loss_cls, zero box terms
    for mine, ref in ((x.grad, [d[f'gcls{l}'] for l in range(5)]), (r.grad, [d[f'greg{l}'] for l in range(5)]),
                      (t.grad[:, None], [d[f'giou{l}'] for l in range(5)])):
        ref = levels_to_flat([T(v) for v in ref]).double()
        assert torch.allclose(mine, ref, rtol=1e-4, atol=1e-7 * float(ref.abs().max()) + 1e-12)      # test_gfl_cpu's bars
    if case != 'n':      # (no positive: the scales are not in the graph)
        assert torch.allclose(s.grad, T(d['gscales']).double(), rtol=1e-4, atol=1e-7)


def test_ref_gmm_reports_a_non_positive_variance():
    """Two well separated samples whose float32 squares round down by more than reg_covar: each component holds one sample, so
    its variance x * x (float32) - mean^2 + 1e-6 comes out negative.  sklearn 1.7.2 raises its ill-defined-covariance error on them."""
    out = PR.gmm_fit(np.array(BAD_SAMPLES, np.float32))
    assert out['flag'] == 2 and out['n_iter'] == 1


@pytest.mark.parametrize('name', 'ab')
def test_ref_detection_equals_reference(golden, name):
    d = golden(f'paa_det_{name}.npz')
    C = int(d['num_classes'])
    assert C == (20 if name == 'a' else 3)
    worst = 0.0
    for i in range(2):
        view = [[T(d[f'{k}{l}'])[i] for l in range(5)] for k in ('cls', 'reg', 'iou')]
        dets, labels, unv = PR.detect_image(*view, T(d['scales']), d['shapes'][i], d['scale_factors'][i], nms_pre=int(d['nms_pre']))
        assert np.array_equal(labels, d[f'labels{i}']) and len(dets) == len(d[f'dets{i}']) >= 10
        assert np.abs(dets[:, 4] - d[f'dets{i}'][:, 4]).max() < 1e-6
        assert np.array_equal(unv, d[f'unvoted{i}'])
        worst = max(worst, float(np.abs(dets[:, :4].astype(np.float64) - d[f'dets{i}'][:, :4]).max()))
        assert bool((np.diff(labels) >= 0).all())      # class ascending, then the NMS's order
        plain, pl, _ = PR.detect_image(*view, T(d['scales']), d['shapes'][i], d['scale_factors'][i], nms_pre=int(d['nms_pre']), score_voting=False)
        assert sorted(zip(pl.tolist(), plain[:, 4].tolist())) == sorted(zip(labels.tolist(), dets[:, 4].tolist()))
    assert worst == pytest.approx(float(d['vote_dev']), rel=1e-6) and worst < 1e-3


# ---- configuration surface ------------------------------------------------------------------------------------------------------
# head, train_cfg and test_cfg of configs/paa/paa_r50_fpn_1x_coco.py, as that file has them
PAA_HEAD = dict(
    type='PAAHead', reg_decoded_bbox=True, score_voting=True, topk=9, num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
    anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1, strides=[8, 16, 32, 64, 128]),
    bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[0.1, 0.1, 0.2, 0.2]),
    loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
    loss_bbox=dict(type='GIoULoss', loss_weight=1.3),
    loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=0.5))
PAA_TRAIN = dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.1, neg_iou_thr=0.1, min_pos_iou=0, ignore_iof_thr=-1),
                 allowed_border=-1, pos_weight=-1, debug=False)
PAA_TEST = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)


def paa_model_cfg(**head):
    cfg = atss_model_cfg()
    cfg['type'] = 'PAA'
    cfg['bbox_head'] = dict(copy.deepcopy(PAA_HEAD), **head)
    cfg['train_cfg'], cfg['test_cfg'] = copy.deepcopy(PAA_TRAIN), copy.deepcopy(PAA_TEST)
    return cfg


def build(cfg=None):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(cfg or paa_model_cfg())


def test_paa_config_builds_on_the_caffe_backbone():
    from dsl_amd import _lib as L
    from dsl_amd.detectors import FCOS, GFL, PAA, ATSSHead, PAAHead
    m = build()
    assert isinstance(m, PAA) and isinstance(m, FCOS) and not isinstance(m, GFL)
    assert isinstance(m.bbox_head, PAAHead) and isinstance(m.bbox_head, ATSSHead)
    o = m.store.head
    assert (o.head_kind, o.assigner, o.atss_topk, o.pos_iou_thr, o.score_voting) == ('paa', 'atss', 9, 0.1, True)
    assert (o.box_loss, o.bbox_weight, o.ctr_weight, o.cls_weight, o.conv_bias) == ('giou', 1.3, 0.5, 1.0, False)
    assert o.flags() == L.HEAD_ATSS | L.HEAD_PAA | L.HEAD_LOSS_EXT and not o.is_default()
    assert m.bbox_head.with_score_voting and m.bbox_head.topk == 9 and m.bbox_head.covariance_type == 'diag'


def test_loss_plan_descriptor_of_a_paa_head():
    import ctypes as C
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    o = HeadOptions(head_kind='paa', atss_topk=3, anchor_scale=4.0, bbox_weight=1.3, pos_iou_thr=0.2)
    p = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o, max_gt=64)
    assert p.paa is not None and C.addressof(p.paa) == C.addressof(p.desc) and p.gfl is None
    assert p.desc.head_flags == L.HEAD_ATSS | L.HEAD_PAA | L.HEAD_LOSS_EXT and p.desc.atss and p.desc.w_bbox == pytest.approx(1.3)
    assert (p.atss.topk, p.atss.max_gt, p.paa.pos_iou_thr) == (3, 64, pytest.approx(0.2)) and p.logvec.numel() == 4
    assert p.paa.pos_loss == p.pos_loss.data_ptr() and p.paa.gmm_flags == p.gmm_flags.data_ptr() and p.gmm_iters.numel() == 64
    assert p.desc.workspace_bytes >= 64 * 12
    with pytest.raises(ValueError, match='pad_shape'):
        p.set_targets([torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2)


def test_descriptor_layout_matches_the_header(tmp_path):
    """dsl_paa_desc's ctypes mirror against the C compiler's layout (tests/test_abi.py's method)."""
    import ctypes
    import os
    import subprocess
    from dsl_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / 'sizes.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsl_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d\\n", sizeof(dsl_paa_desc), offsetof(dsl_paa_desc, pos_iou_thr), offsetof(dsl_paa_desc, gmm_flags), '
                   'DSL_HEAD_PAA, DSL_OP_PAA_REFINE);\n  return 0;\n}\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out == [ctypes.sizeof(L.PaaDesc), L.PaaDesc.pos_iou_thr.offset, L.PaaDesc.gmm_flags.offset, L.HEAD_PAA, L.OP_PAA_REFINE]
    assert L.HEAD_PAA == 256 and not L.MISSING


def _with(path, value):
    cfg = paa_model_cfg()
    node = cfg
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value
    return cfg


@pytest.mark.parametrize('path,value,word', [
    (('bbox_head', 'topk'), 17, 'topk'),
    (('bbox_head', 'topk'), 0, 'topk'),
    (('bbox_head', 'covariance_type'), 'full', 'covariance_type'),
    (('bbox_head', 'covariance_type'), 'spherical', 'covariance_type'),
    (('bbox_head', 'reg_decoded_bbox'), False, 'reg_decoded_bbox'),
    (('bbox_head', 'anchor_generator', 'ratios'), [0.5, 1.0, 2.0], 'ratios'),
    (('bbox_head', 'bbox_coder', 'type'), 'TBLRBBoxCoder', 'DeltaXYWHBBoxCoder'),
    (('bbox_head', 'stacked_convs'), 2, 'stacked_convs'),
    (('bbox_head', 'soft_weight'), 1.0, 'soft_weight'),
    (('train_cfg', 'assigner', 'type'), 'ATSSAssigner', 'MaxIoUAssigner'),
    (('train_cfg', 'assigner', 'neg_iou_thr'), 0.05, 'neg_iou_thr'),
    (('train_cfg', 'assigner', 'pos_iou_thr'), 1.0, 'pos_iou_thr'),
    (('train_cfg', 'assigner', 'min_pos_iou'), 0.05, 'min_pos_iou'),
    (('train_cfg', 'assigner', 'ignore_iof_thr'), 0.5, 'ignore_iof_thr'),
    (('train_cfg', 'assigner', 'gt_max_assign_all'), False, 'gt_max_assign_all'),
    (('train_cfg', 'assigner', 'match_low_quality'), False, 'match_low_quality'),
    (('train_cfg', 'assigner', 'gpu_assign_thr'), 100, 'gpu_assign_thr'),
    (('train_cfg', 'assigner', 'topk'), 9, 'topk'),
    (('train_cfg', 'allowed_border'), 0, 'allowed_border'),
    (('train_cfg', 'pos_weight'), 2.0, 'pos_weight'),
])
def test_refused_options_are_named(path, value, word):
    with pytest.raises(NotImplementedError, match=word):
        build(_with(path, value))


def test_fp8_towers_and_other_heads_stay_refused():
    from dsl_amd.registry import build_detector
    with pytest.raises(NotImplementedError, match='fp8 towers'):
        build_detector(dict(paa_model_cfg(), fp8=dict(layers='towers')))
    cfg = paa_model_cfg()
    cfg['bbox_head'] = atss_model_cfg()['bbox_head']
    with pytest.raises(NotImplementedError, match='PAAHead'):
        build_detector(cfg)
    cfg = atss_model_cfg()
    cfg['bbox_head'], cfg['train_cfg'] = copy.deepcopy(PAA_HEAD), copy.deepcopy(PAA_TRAIN)
    with pytest.raises(NotImplementedError, match='ATSSHead'):
        build_detector(cfg)


def test_existing_head_keys_and_descriptors_are_unchanged():
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    assert HeadOptions().key() == (True, True, True, False, True) and HeadOptions().flags() == 0
    k = HeadOptions(assigner='atss').key()
    assert k[:5] == (True, True, True, False, False) and k[5:] == ('atss', 9, 8.0, (0.1, 0.1, 0.2, 0.2))
    assert HeadOptions(assigner='atss', bbox_weight=2.0).flags() == L.HEAD_ATSS | L.HEAD_LOSS_EXT
    g = HeadOptions(head_kind='gfl')
    assert g.key()[-4:] == ('gfl', 16, 2.0, 0.25) and g.flags() == L.HEAD_ATSS | L.HEAD_GFL | L.HEAD_LOSS_EXT
    assert 'pos_iou_thr' not in repr(g) and 'pos_iou_thr' not in repr(HeadOptions(assigner='atss'))
    p = HeadOptions(head_kind='paa')
    assert p.key()[-3:] == ('paa', 0.1, True) and p.key()[:-3] == k and p.flags() == L.HEAD_ATSS | L.HEAD_PAA | L.HEAD_LOSS_EXT
    for o in (HeadOptions(assigner='atss'), g):
        lp = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o, max_gt=64)
        assert lp.paa is None and not lp.desc.head_flags & L.HEAD_PAA and not hasattr(lp, 'pos_loss')
    with pytest.raises(NotImplementedError, match='head_kind'):
        HeadOptions(head_kind='vfnet')
    with pytest.raises(NotImplementedError, match='pos_iou_thr'):
        HeadOptions(head_kind='paa', pos_iou_thr=0.0)
    with pytest.raises(NotImplementedError, match='atss_topk'):
        HeadOptions(head_kind='paa', atss_topk=17)


def test_state_dict_names_round_trip():
    m = build()
    sd = m.state_dict()
    from test_atss_cpu import build as build_atss
    assert list(sd) == list(build_atss().state_dict())      # ATSSHead's keys, in its order
    names = ('bbox_head.atss_cls', 'bbox_head.atss_reg', 'bbox_head.atss_centerness')
    assert [tuple(sd[f'{n}.weight'].shape) for n in names] == [(80, 256, 3, 3), (4, 256, 3, 3), (1, 256, 3, 3)]
    g = torch.Generator().manual_seed(5)
    new = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    m.load_state_dict(copy.deepcopy(new))
    out = m.state_dict()
    for k, v in new.items():
        assert torch.equal(out[k], v), k
