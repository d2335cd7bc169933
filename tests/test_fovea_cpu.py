"""FoveaBox without a GPU: tests/fovea_ref.py against what the reference's own FoveaHead computed (tests/golden/fovea_*.npz, written by
tests/golden/make_fovea_golden.py), the configuration surface of HeadOptions(head_kind='fovea') / FoveaHead / FOVEA, and the records
of the head kinds that existed before it."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import fovea_ref as FR
from util import fcos_model_cfg

T = torch.from_numpy
CASES = 'abcde'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

FOVEA_HEAD = dict(type='FoveaHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256, strides=[8, 16, 32, 64, 128],
                  base_edge_list=[16, 32, 64, 128, 256], scale_ranges=((1, 64), (32, 128), (64, 256), (128, 512), (256, 2048)), sigma=0.4,
                  with_deform=False, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                  loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.50, alpha=0.4, loss_weight=1.0),
                  loss_bbox=dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0))
FOVEA_TEST = dict(nms_pre=1000, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)


def fovea_model_cfg(**head):
    """configs/foveabox/fovea_r50_fpn_4x4_1x_coco.py's bbox_head (with GN-32 towers) and test_cfg on the caffe ResNet-50 + this FPN."""
    cfg = fcos_model_cfg()
    cfg['type'] = 'FOVEA'
    cfg['bbox_head'] = dict(copy.deepcopy(FOVEA_HEAD), **head)
    cfg['train_cfg'], cfg['test_cfg'] = dict(), copy.deepcopy(FOVEA_TEST)
    return cfg


def build(cfg=None):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(cfg or fovea_model_cfg())


@functools.lru_cache(maxsize=None)
def load_case(case):
    d = np.load(os.path.join(GOLDEN, f'fovea_{case}.npz'))
    B, C = int(d['B']), int(d['num_classes'])
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    c = dict(d=d, B=B, C=C, sizes=sizes, sigma=float(d['sigma']), base=tuple(float(v) for v in d['base_edge_list']),
             ranges=tuple((float(lo), float(hi)) for lo, hi in d['scale_ranges']), beta=float(d['beta']), gamma=float(d['gamma']),
             alpha=float(d['alpha']), cls_weight=float(d['cls_weight']), bbox_weight=float(d['bbox_weight']),
             gts=[T(d[f'gt{i}']) for i in range(B)], gls=[T(d[f'gl{i}']) for i in range(B)],
             cls=[T(d[f'cls{l}']) for l in range(5)], reg=[T(d[f'reg{l}']) for l in range(5)])
    c['asg'] = FR.assign(c['gts'], c['gls'], sizes, C, c['sigma'], c['base'], c['ranges'])
    return c


@functools.lru_cache(maxsize=None)
def ref_loss(case):
    """(loss_cls, loss_bbox, d/dcls [M, C], d/dreg [M, 4]) of fovea_ref in float64: computed once, shared by the tests."""
    c = load_case(case)
    cls, reg = FR.flat(c['cls']).double().requires_grad_(), FR.flat(c['reg']).double().requires_grad_()
    lc, lb = FR.loss(cls, reg, c['asg'], c['B'], c['C'], c['gamma'], c['alpha'], c['beta'], c['cls_weight'], c['bbox_weight'])
    (lc + lb).backward()
    return float(lc.detach()), float(lb.detach()), cls.grad, reg.grad


@pytest.mark.parametrize('case', CASES)
def test_ref_assignment_equals_the_reference(case):
    c = load_case(case)
    d, a = c['d'], c['asg']
    assert torch.equal(a['labels'], T(d['labels']))
    assert torch.equal(a['assign_idx'], T(d['assign_idx']))
    assert a['num_pos'] == int(d['num_pos'])
    pos = T(d['pos'])
    assert torch.equal((a['labels'] < c['C']).nonzero().view(-1), pos)
    if len(pos):
        # four fp32 ulps at log 16 = 2.77
        assert float((a['targets'][pos] - T(d['log_targets'])).abs().max()) <= 1e-6
    keep = torch.ones(len(a['labels']), dtype=torch.bool)
    keep[pos] = False
    assert not bool(a['targets'][keep].any())
    assert a['stats'] == (float(a['num_pos'] + c['B']), float(max(a['num_pos'], 1)))


def test_fixture_cases_hold_what_they_are_for():
    b, c, dd, e = (load_case(k) for k in 'bcde')
    assert list(b['d']['npos_img'])[1] == 0 and int(b['d']['num_pos']) > 0
    assert int(c['d']['num_pos']) == 0 and float(c['d']['loss_bbox']) == 0.0
    assert not any(bool(T(c['d'][f'greg{l}']).any()) for l in range(5))
    i0 = T(dd['d']['assign_idx'])[:320].reshape(16, 20)
    assert all(bool((i0 == g).any()) for g in (0, 1, 2)) and not bool((i0 == 3).any())          # nested boxes; the empty fovea
    assert int(i0[15, 19]) == 4 and int((i0 == 4).sum()) == 1                                    # beyond both edges: the corner cell
    assert bool((T(dd['d']['assign_idx'])[640:720] == 0).any())                                   # box 0 on level 1 too
    lab, o = T(e['d']['labels']), 0
    for h, w in e['sizes']:
        assert bool((lab[o:o + 2 * h * w] < e['C']).any())
        o += 2 * h * w
    assert e['C'] == 18 and e['sigma'] == 0.25 and e['beta'] == 1.0


@pytest.mark.parametrize('case', CASES)
def test_ref_loss_equals_the_reference(case):
    c = load_case(case)
    d = c['d']
    lc, lb, gc, gr = ref_loss(case)
    assert lc == pytest.approx(float(d['loss_cls']), rel=1e-5)
    assert lb == pytest.approx(float(d['loss_bbox']), rel=1e-5, abs=0.0 if case == 'c' else 1e-12)
    want_c, want_r = FR.flat([T(d[f'gcls{l}']) for l in range(5)]).double(), FR.flat([T(d[f'greg{l}']) for l in range(5)]).double()
    assert float((gc - want_c).abs().max()) <= 1e-4 * max(float(want_c.abs().max()), 1e-30)
    assert float((gr - want_r).abs().max()) <= 1e-4 * max(float(want_r.abs().max()), 1e-30)
    if case == 'c':
        assert lb == 0.0 and not bool(gr.any())


@pytest.mark.parametrize('case', CASES)
def test_ref_detection_equals_the_reference(case):
    c = load_case(case)
    d = c['d']
    cls, reg = [x.double() for x in c['cls']], [x.double() for x in c['reg']]
    out = FR.detect(cls, reg, [tuple(s) for s in d['img_shapes']], list(d['scale_factors']), nms_pre=int(d['nms_pre']),
                    score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']), base=c['base'])
    for i, (dets, labels) in enumerate(out):
        want_b, want_l = T(d[f'det{i}_boxes']).double(), T(d[f'det{i}_labels'])
        assert dets.shape == want_b.shape and torch.equal(labels, want_l)          # the same kept set in the same order
        assert float((dets[:, :4] - want_b[:, :4]).abs().max()) <= 1e-4
        assert float((dets[:, 4] - want_b[:, 4]).abs().max()) <= 1e-6
    # the second image is smaller than the canvas: the clamp to img_shape - 1 bites (in the view's frame: times the scale factor)
    b1 = T(d['det1_boxes'])[:, :4] * float(d['scale_factors'][1][0])
    assert float(b1[:, 2].max()) == pytest.approx(float(d['img_shapes'][1][1]) - 1, abs=1e-3)


# ---- HeadOptions(head_kind='fovea') ----------------------------------------------------------------------------------------------
def test_head_options_key_repr_layout():
    from dsl_amd import _lib as L
    from dsl_amd.params import HEAD_KINDS, HeadOptions
    o = HeadOptions(head_kind='fovea')
    assert o.kind is HEAD_KINDS['fovea'] and o.assigner == 'fcos'
    assert o.key() == (True, True, True, False, True, 'fovea', 0.4, (16.0, 32.0, 64.0, 128.0, 256.0),
                       ((8.0, 32.0), (16.0, 64.0), (32.0, 128.0), (64.0, 256.0), (128.0, 512.0)), 0.11)
    assert repr(o) == ('HeadOptions(center_sampling=True, norm_on_bbox=True, centerness_on_reg=True, iou_loss=False, conv_bias=True, '
                       'head_kind=fovea, sigma=0.4, base_edge_list=(16.0, 32.0, 64.0, 128.0, 256.0), scale_ranges=((8.0, 32.0), (16.0, 64.0), '
                       '(32.0, 128.0), (64.0, 256.0), (128.0, 512.0)), smooth_l1_beta=0.11)')
    assert o.reg_layout() == (4, 8) and not o.has_scale() and not o.is_default()
    assert o.flags() == L.HEAD_FOVEA | L.HEAD_LOSS_EXT == 528
    p = HeadOptions(head_kind='fovea', sigma=0.25, base_edge_list=(8, 16, 32, 64, 128), scale_ranges=((1, 16), (8, 32), (16, 64), (32, 128), (64, 512)),
                    smooth_l1_beta=1.0, conv_bias=False, focal_gamma=1.5, focal_alpha=0.4, cls_weight=2.0, bbox_weight=0.5)
    assert p.key() != o.key() and p.key()[5:12] == ('giou', 1e-6, 1.5, 0.4, 2.0, 0.5, 1.0) and p.key()[12:14] == ('fovea', 0.25)
    assert (p.range_lo, p.range_hi) == ((1.0, 8.0, 16.0, 32.0, 64.0), (16.0, 32.0, 64.0, 128.0, 512.0))
    k = o.kind
    assert (k.atss, k.loss_desc, k.det_desc, k.names, k.middle, k.loss_entry, k.loss_keys, k.sisoft, k.exchange) == \
        (False, ('FoveaDesc', 'fovea'), ('DetFoveaDesc', 'det'), ('conv_cls', 'conv_reg', None), None, 'dsl_fovea_loss',
         ('loss_cls', 'loss_bbox'), False, None)
    assert 'no with_nms argument' in k.aug_refusal and 'dense_test_mixins.py:62-70' in k.aug_refusal


REFUSED = [dict(center_sampling=False), dict(norm_on_bbox=False), dict(centerness_on_reg=False), dict(iou_loss=True), dict(box_loss='diou'),
           dict(ctr_weight=0.5), dict(assigner='atss'), dict(atss_topk=5), dict(anchor_scale=4.0), dict(delta_stds=(1.0, 1.0, 1.0, 1.0)),
           dict(reg_max=8), dict(qfl_beta=1.0), dict(dfl_weight=0.5), dict(ld_weight=0.25), dict(ld_T=4.0), dict(pos_iou_thr=0.2),
           dict(score_voting=False), dict(sigma=0.0), dict(sigma=1.5), dict(smooth_l1_beta=0.0), dict(base_edge_list=(16, 32, 64, 128)),
           dict(base_edge_list=(16, 32, 64, 128, 0)), dict(scale_ranges=((8, 32),) * 4), dict(scale_ranges=((32, 8),) * 5)]


@pytest.mark.parametrize('kw', REFUSED, ids=lambda kw: next(iter(kw)) + '=' + str(next(iter(kw.values()))))
def test_head_options_refusals(kw):
    from dsl_amd.params import HeadOptions
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        HeadOptions(head_kind='fovea', **kw)


def test_head_kind_name_is_checked():
    from dsl_amd.params import HeadOptions
    with pytest.raises(NotImplementedError, match="'fovea'"):
        HeadOptions(head_kind='retina')


# ---- FoveaHead / FOVEA -----------------------------------------------------------------------------------------------------------
def test_fovea_config_builds_with_the_references_keys():
    from dsl_amd.detectors import FCOS, FOVEA, FoveaHead
    m = build()
    assert isinstance(m, FOVEA) and isinstance(m, FCOS) and isinstance(m.bbox_head, FoveaHead)
    o = m.store.head
    assert (o.head_kind, o.sigma, o.smooth_l1_beta, o.focal_gamma, o.focal_alpha, o.conv_bias) == ('fovea', 0.4, 0.11, 1.5, 0.4, False)
    assert o.scale_ranges[0] == (1.0, 64.0) and o.base_edge_list[4] == 256.0
    sd = m.state_dict()
    head = [k for k in sd if k.startswith('bbox_head.')]
    assert sorted(head) == sorted(str(k) for k in load_case('a')['d']['head_keys'])
    assert sd['bbox_head.conv_reg.weight'].shape == (4, 256, 3, 3) and sd['bbox_head.conv_cls.weight'].shape == (80, 256, 3, 3)
    assert (m.store.reg_rows, m.store.reg_ld, m.store.reg_pad) == (4, 8, 64) and 'head.scales' not in m.store.train_regions
    # init_cfg: Normal(0, 0.01), conv_cls's bias from bias_prob = 0.01
    assert float(sd['bbox_head.conv_cls.bias'][0]) == pytest.approx(-np.log(99.0), rel=1e-6)
    assert 0.008 < float(sd['bbox_head.conv_reg.weight'].std()) < 0.012 and not bool(sd['bbox_head.conv_reg.bias'].any())
    m2 = build()
    m2.load_state_dict({k: v + 1 if v.dtype.is_floating_point else v for k, v in sd.items()})
    assert torch.equal(m2.state_dict()['bbox_head.conv_reg.bias'], sd['bbox_head.conv_reg.bias'] + 1)


BAD_HEADS = [(dict(with_deform=True), 'with_deform'), (dict(stacked_convs=3), 'stacked_convs'), (dict(norm_cfg=None), 'GN-32'),
             (dict(norm_cfg=dict(type='BN')), 'GN-32'), (dict(strides=[4, 8, 16, 32, 64]), 'strides'),
             (dict(loss_bbox=dict(type='GIoULoss')), 'SmoothL1Loss'), (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True)), 'FocalLoss'),
             (dict(dcn_on_last_conv=True), 'DCN'), (dict(soft_weight=0.1), 'soft_weight'), (dict(sigma=2.0), 'sigma')]


@pytest.mark.parametrize('head,what', BAD_HEADS, ids=[w + str(i) for i, (_, w) in enumerate(BAD_HEADS)])
def test_fovea_head_refusals(head, what):
    with pytest.raises(NotImplementedError, match=what):
        build(fovea_model_cfg(**head))


def test_fovea_detector_wants_a_fovea_head():
    cfg = fovea_model_cfg()
    cfg['bbox_head'] = fcos_model_cfg()['bbox_head']
    with pytest.raises(NotImplementedError, match='FoveaHead'):
        build(cfg)
    with pytest.raises(NotImplementedError, match='fp8'):
        build(dict(fovea_model_cfg(), fp8=dict(layers='towers')))


def test_aug_test_is_refused():
    m = build()
    with pytest.raises(NotImplementedError, match='with_nms'):
        m.aug_test([torch.zeros(1, 3, 64, 96)] * 2, [[dict()], [dict()]])


def test_smooth_l1_stays_refused_by_the_other_heads():
    from test_atss_cpu import atss_model_cfg
    cfg = atss_model_cfg()
    cfg['bbox_head']['loss_bbox'] = dict(type='SmoothL1Loss', beta=0.11, loss_weight=1.0)
    with pytest.raises(NotImplementedError):
        build(cfg)


# ---- the kinds that existed before -----------------------------------------------------------------------------------------------
KIND_REPRS = {
    'fcos': "HeadKind(name='fcos', flags=0, atss=False, fields=(), loss_desc=('FcosDesc',), scalars=(), buffers=(), det_desc=('DetDesc',), det_mask=4, det_fields=(), dist_reg=False, names=('conv_cls', 'conv_reg', 'conv_centerness'), middle=None, loss_entry='dsl_fcos_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_centerness'), sisoft=True, exchange='forward', aug_refusal=None)",
    'atss': "HeadKind(name='atss', flags=32, atss=True, fields=('assigner', 'atss_topk', 'anchor_scale', 'delta_stds'), loss_desc=('FcosDesc',), scalars=(), buffers=(), det_desc=('DetAtssDesc', 'det'), det_mask=36, det_fields=(), dist_reg=False, names=('atss_cls', 'atss_reg', 'atss_centerness'), middle=None, loss_entry='dsl_fcos_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_centerness'), sisoft=True, exchange='forward', aug_refusal=None)",
    'gfl': "HeadKind(name='gfl', flags=112, atss=True, fields=('assigner', 'atss_topk', 'anchor_scale', 'delta_stds', 'head_kind', 'reg_max', 'qfl_beta', 'dfl_weight'), loss_desc=('GflDesc', 'gfl'), scalars=(('gfl', 'reg_max', 'reg_max'), ('gfl', 'qfl_beta', 'qfl_beta'), ('gfl', 'w_dfl', 'dfl_weight')), buffers=(('score', torch.float32, 'M', 0), ('weight', torch.float32, 'M', 0)), det_desc=('DetGflDesc', 'det'), det_mask=64, det_fields=(('reg_max', 'reg_max'),), dist_reg=True, names=('gfl_cls', 'gfl_reg', None), middle=(29, ('dsl_gfl_quality',)), loss_entry='dsl_gfl_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_dfl'), sisoft=False, exchange='middle', aug_refusal=None)",
    'ld': "HeadKind(name='ld', flags=240, atss=True, fields=('assigner', 'atss_topk', 'anchor_scale', 'delta_stds', 'head_kind', 'reg_max', 'qfl_beta', 'dfl_weight', 'ld_weight', 'ld_T'), loss_desc=('LdDesc', 'ld', 'gfl'), scalars=(('gfl', 'reg_max', 'reg_max'), ('gfl', 'qfl_beta', 'qfl_beta'), ('gfl', 'w_dfl', 'dfl_weight'), ('ld', 'T', 'ld_T'), ('ld', 'w_ld', 'ld_weight')), buffers=(('score', torch.float32, 'M', 0), ('weight', torch.float32, 'M', 0)), det_desc=('DetGflDesc', 'det'), det_mask=64, det_fields=(('reg_max', 'reg_max'),), dist_reg=True, names=('gfl_cls', 'gfl_reg', None), middle=(29, ('dsl_gfl_quality',)), loss_entry='dsl_ld_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld'), sisoft=False, exchange='middle', aug_refusal=None)",
    'paa': "HeadKind(name='paa', flags=304, atss=True, fields=('assigner', 'atss_topk', 'anchor_scale', 'delta_stds', 'head_kind', 'pos_iou_thr', 'score_voting'), loss_desc=('PaaDesc', 'paa'), scalars=(('paa', 'pos_iou_thr', 'pos_iou_thr'),), buffers=(('pos_loss', torch.float32, 'M', 0), ('iou_target', torch.float32, 'M', 0), ('cand_gt', torch.int32, 'M', -1), ('gmm_iters', torch.int32, 'max_gt', 0), ('gmm_flags', torch.int32, 'max_gt', 0)), det_desc=('DetPaaDesc', 'atss', 'det'), det_mask=292, det_fields=(('score_voting', 'score_voting'),), dist_reg=False, names=('atss_cls', 'atss_reg', 'atss_centerness'), middle=(30, ('dsl_paa_pos_loss', 'dsl_paa_reassign')), loss_entry='dsl_paa_loss', loss_keys=('loss_cls', 'loss_bbox', 'loss_iou'), sisoft=False, exchange=None, aug_refusal='PAAHead does not support test-time augmentation (aug_test): PAA only supports with_nms=True (paa_head.py:536-538)')",
}


@pytest.mark.parametrize('name', sorted(KIND_REPRS))
def test_existing_head_kinds_are_unchanged(name):
    from dsl_amd.params import HEAD_KINDS
    assert repr(HEAD_KINDS[name]) == KIND_REPRS[name]
