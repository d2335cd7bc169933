"""AutoAssign without a GPU: tests/autoassign_ref.py against what the reference's own AutoAssignHead computed
(tests/golden/autoassign_*.npz, written by tests/golden/make_autoassign_golden.py), what fp32 itself holds of the prior's gradients,
and the configuration surface of HeadOptions(head_kind='autoassign') / AutoAssignHead / AutoAssign."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import autoassign_ref as AR
from util import fcos_model_cfg

T = torch.from_numpy
CASES = 'abcde'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# configs/autoassign/autoassign_r50_fpn_8x2_1x_coco.py, verbatim
AA_HEAD = dict(type='AutoAssignHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256, strides=[8, 16, 32, 64, 128],
               loss_bbox=dict(type='GIoULoss', loss_weight=5.0))
AA_TEST = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)


def aa_model_cfg(**head):
    """The config's bbox_head and test_cfg on the caffe ResNet-50 + this project's FPN (its neck, add_extra_convs on the input, is not
    built: DESIGN section 7)."""
    cfg = fcos_model_cfg()
    cfg['type'] = 'AutoAssign'
    cfg['bbox_head'] = dict(copy.deepcopy(AA_HEAD), **head)
    cfg['train_cfg'], cfg['test_cfg'] = None, copy.deepcopy(AA_TEST)
    return cfg


def build(cfg=None):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(cfg or aa_model_cfg())


@functools.lru_cache(maxsize=None)
def load_case(case):
    d = np.load(os.path.join(GOLDEN, f'autoassign_{case}.npz'))
    B, C = int(d['B']), int(d['num_classes'])
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    return dict(d=d, B=B, C=C, sizes=sizes, pos_w=float(d['pos_loss_weight']), neg_w=float(d['neg_loss_weight']),
                center_w=float(d['center_loss_weight']), bbox_weight=float(d['bbox_weight']),
                gts=[T(d[f'gt{i}']) for i in range(B)], gls=[T(d[f'gl{i}']) for i in range(B)],
                cls=AR.flat([T(d[f'cls{l}']) for l in range(5)]), raw=AR.flat([T(d[f'raw{l}']) for l in range(5)]),
                obj=AR.flat([T(d[f'obj{l}']) for l in range(5)]), scales=T(d['scales']), mean=T(d['mean']), sigma=T(d['sigma']))


def run_ref(case, dtype):
    """autoassign_ref's losses and gradients in `dtype`: (out dict, d/dcls, d/dbbox_pred, d/draw, d/dobj, d/dscales, d/dmean, d/dsigma)."""
    c = load_case(case)
    leaf = lambda t: t.to(dtype).clone().requires_grad_()      # noqa: E731
    cls, raw, obj, sc, mean, sigma = (leaf(c[k]) for k in ('cls', 'raw', 'obj', 'scales', 'mean', 'sigma'))
    out = AR.loss(cls, raw, obj, sc, mean, sigma, c['gts'], c['gls'], c['sizes'], c['C'], c['pos_w'], c['neg_w'], c['center_w'], c['bbox_weight'])
    (out['loss_pos'] + out['loss_neg'] + out['loss_center']).backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)      # noqa: E731
    return out, z(cls), z(raw), z(obj), z(sc), z(mean), z(sigma)


@functools.lru_cache(maxsize=None)
def ref_loss(case):
    """float64, computed once and shared by the tests"""
    return run_ref(case, torch.float64)


def bbox_grad_to_raw(c, gbbox):
    """The fixture's gradient with respect to bbox_pred = relu(scale x) s taken to conv_reg's output and the Scale values, float64."""
    _, lvl, _ = AR.flat_points(c['sizes'], c['B'])
    s = T(np.asarray(AR.STRIDES, np.float64)[lvl])[:, None]
    sc = c['scales'].double()[T(lvl)][:, None]
    raw = c['raw'].double()
    on = (raw * sc > 0).double()
    graw = gbbox * s * on * sc
    gsc = torch.zeros(5, dtype=torch.float64).index_add_(0, T(lvl), (gbbox * s * on * raw).sum(1))
    return graw, gsc


def close(got, want, rel=1e-4):
    return float((got - want).abs().max()) <= rel * max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize('case', CASES)
def test_ref_assignment_equals_the_reference(case):
    c = load_case(case)
    d = c['d']
    out = ref_loss(case)[0]
    for i in range(c['B']):
        ins = T(d[f'inside{i}'])
        assert torch.equal(out['inside'][i], ins)                                                   # exact
        assert close(out['prior'][i][ins], T(d[f'prior{i}']).double(), 1e-5) if bool(ins.any()) else not bool(out['prior'][i].any())
        assert not bool(out['prior'][i][~ins].any())
        assert float((out['iou'][i] - T(d[f'iou{i}']).double()).abs().max()) <= 1e-5
        want = T(d[f'negw{i}']).double()
        # (the same-class winner - the highest box index - is checked on case d's shared points below)
        assert float((out['negw'][i] - want).abs().max()) <= 1e-4


def test_fixture_cases_hold_what_they_are_for():
    a, b, c, dd, e = (load_case(k) for k in CASES)
    assert a['C'] == 80 and bool((a['mean'] != 0).all()) and bool((a['sigma'] != 1).all())
    assert len(b['gts'][1]) == 0 and len(b['gts'][0]) > 0
    assert len(c['gts'][0]) == len(c['gts'][1]) == 0 and float(c['d']['loss_pos']) == 0.0 and float(c['d']['loss_center']) == 0.0
    assert not bool(T(c['d']['gmean']).any()) and not bool(T(c['d']['gsigma']).any())
    ins = T(dd['d']['inside0'])
    assert list(dd['gls'][0]) == [3, 3, 7, 3, 5]
    assert not bool(ins[:, 3].any()) and bool(ins[:, 4].all()) and bool((ins[:, 0] & ins[:, 1]).any())
    # R = 0 for the box without a point: its term is the clamp's 100, times pos_loss_weight over the batch's 9 boxes
    out = ref_loss('d')[0]
    assert float(out['R'][0][3]) == 0.0
    R = torch.cat(out['R'])
    terms = torch.where(R > 0, -torch.log(R.clamp(min=1e-300)), torch.full_like(R, 100.0))
    assert float(terms[3]) == 100.0 and float(dd['d']['loss_pos']) == pytest.approx(float(0.25 * terms.sum() / 9.0), rel=1e-5)
    # the shared points of boxes 0 and 1 (class 3) carry box 1's weight
    both = ins[:, 0] & ins[:, 1]
    iou = T(dd['d']['iou0']).double()
    t = 1 / (1 - iou[ins[:, 1]]).clamp(min=1e-12)
    w1 = torch.ones(len(iou), dtype=torch.float64)
    w1[ins[:, 1]] = 1 - (t - t.min() + 1e-12) / (t.max() - t.min() + 1e-12)
    assert float((T(dd['d']['negw0']).double()[both, 3] - w1[both]).abs().max()) <= 1e-4
    assert (e['C'], e['pos_w'], e['neg_w'], e['center_w'], e['bbox_weight']) == (18, 0.5, 1.5, 0.3, 2.0)


@pytest.mark.parametrize('case', CASES)
def test_ref_loss_equals_the_reference(case):
    c = load_case(case)
    d = c['d']
    out, gc, gr, go, gs, gm, gsg = ref_loss(case)
    for k in ('loss_pos', 'loss_neg', 'loss_center'):
        assert float(out[k].detach()) == pytest.approx(float(d[k]), rel=1e-5, abs=0.0 if float(d[k]) == 0.0 else 1e-12), k
    want_c, want_o = AR.flat([T(d[f'gcls{l}']) for l in range(5)]).double(), AR.flat([T(d[f'gobj{l}']) for l in range(5)]).double()
    want_r, _ = bbox_grad_to_raw(c, AR.flat([T(d[f'gbbox{l}']) for l in range(5)]).double())
    assert close(gc, want_c) and close(go, want_o) and close(gr, want_r)
    assert close(gm, T(d['gmean']).double()) and close(gsg, T(d['gsigma']).double())
    if case == 'c':
        assert not bool(gr.any()) and not bool(gm.any()) and not bool(gsg.any())


@pytest.mark.parametrize('case', CASES)
def test_ref_detection_equals_the_reference(case):
    c = load_case(case)
    d = c['d']
    n = c['B']
    cls, raw, obj = (AR.unflat(c[k].double(), c['sizes'], n) for k in ('cls', 'raw', 'obj'))
    out = AR.detect(cls, raw, obj, c['scales'].double(), [tuple(s) for s in d['img_shapes']], list(d['scale_factors']), nms_pre=int(d['nms_pre']),
                    score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']))
    for i, (dets, labels) in enumerate(out):
        want_b, want_l = T(d[f'det{i}_boxes']).double(), T(d[f'det{i}_labels'])
        assert dets.shape == want_b.shape and torch.equal(labels, want_l)          # the same kept set in the same order
        assert float((dets[:, :4] - want_b[:, :4]).abs().max()) <= 1e-4
        assert float((dets[:, 4] - want_b[:, 4]).abs().max()) <= 1e-6


@pytest.mark.parametrize('case', 'abde')
def test_fp32_holds_the_prior_gradient_bar(case):
    """The bar the GPU test sets for d mean / d sigma (1e-4 of the tensor's largest magnitude) is one fp32 arithmetic itself holds:
    the same model in float32 against float64."""
    _, _, _, _, _, gm64, gs64 = ref_loss(case)
    _, _, _, _, _, gm32, gs32 = run_ref(case, torch.float32)
    assert close(gm32.double(), gm64) and close(gs32.double(), gs64)


# ---- HeadOptions(head_kind='autoassign') -----------------------------------------------------------------------------------------
def test_head_kind_record_and_options():
    from dsl_amd import _lib as L
    from dsl_amd.params import HEAD_KINDS, HeadOptions
    k = HEAD_KINDS['autoassign']
    assert list(HEAD_KINDS) == ['fcos', 'atss', 'gfl', 'ld', 'paa', 'fovea', 'autoassign']
    assert (k.flags, k.atss, k.loss_desc, k.det_desc, k.det_mask, k.names, k.middle, k.loss_entry, k.loss_keys, k.sisoft, k.exchange,
            k.aug_refusal) == (L.HEAD_AUTOASSIGN | L.HEAD_LOSS_EXT, False, ('AaDesc', 'aa'), ('DetDesc',), L.HEAD_AUTOASSIGN,
                               ('conv_cls', 'conv_reg', 'conv_centerness'), None, 'dsl_aa_loss', ('loss_pos', 'loss_neg', 'loss_center'),
                               False, 'forward', None)
    assert L.HEAD_AUTOASSIGN == 1024 and k._fields == HEAD_KINDS['fcos']._fields          # no new field
    o = HeadOptions(head_kind='autoassign')
    assert o.kind is k and o.has_scale() and o.has_prior() and not HeadOptions().has_prior() and not o.is_default()
    assert o.flags() == 1040 and o.reg_layout() == (5, 8) and o.conv_bias
    assert (o.pos_loss_weight, o.neg_loss_weight, o.center_loss_weight) == (0.25, 0.75, 0.75)
    assert o.key() == (True, True, True, False, True, 'autoassign', 0.25, 0.75, 0.75)
    p = HeadOptions(head_kind='autoassign', bbox_weight=5.0, box_loss='giou', pos_loss_weight=0.5, neg_loss_weight=1.5, center_loss_weight=0.3)
    assert p.key()[5:] == ('giou', 1e-6, 2.0, 0.25, 1.0, 5.0, 1.0, 'autoassign', 0.5, 1.5, 0.3) and p.key() != o.key()


REFUSED = [dict(center_sampling=False), dict(norm_on_bbox=False), dict(centerness_on_reg=False), dict(iou_loss=True), dict(conv_bias=False),
           dict(box_loss='diou'), dict(box_loss='iou'), dict(box_eps=1e-3), dict(focal_gamma=1.5), dict(focal_alpha=0.4), dict(cls_weight=2.0),
           dict(ctr_weight=0.5), dict(assigner='atss'), dict(atss_topk=5), dict(anchor_scale=4.0), dict(delta_stds=(1.0, 1.0, 1.0, 1.0)),
           dict(reg_max=8), dict(qfl_beta=1.0), dict(dfl_weight=0.5), dict(ld_weight=0.25), dict(ld_T=4.0), dict(pos_iou_thr=0.2),
           dict(score_voting=False), dict(sigma=0.3), dict(base_edge_list=(8, 16, 32, 64, 128)), dict(scale_ranges=((1, 2),) * 5),
           dict(smooth_l1_beta=1.0), dict(bbox_weight=-1.0), dict(bbox_weight=float('inf')), dict(bbox_weight=float('nan')),
           dict(pos_loss_weight=-1.0), dict(neg_loss_weight=float('inf')), dict(center_loss_weight='x')]


@pytest.mark.parametrize('kw', REFUSED, ids=lambda kw: next(iter(kw)) + '=' + str(next(iter(kw.values()))))
def test_head_options_refusals(kw):
    from dsl_amd.params import HeadOptions
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        HeadOptions(head_kind='autoassign', **kw)


def test_the_new_options_belong_to_the_new_kind():
    from dsl_amd.params import HeadOptions
    assert 'pos_loss_weight' not in repr(HeadOptions()) and 'pos_loss_weight' not in repr(HeadOptions(head_kind='fovea'))
    with pytest.raises(NotImplementedError, match="'fovea' or 'autoassign'"):
        HeadOptions(head_kind='retina')


# ---- AutoAssignHead / AutoAssign -------------------------------------------------------------------------------------------------
def test_registry_names():
    """Fails without the feature: neither name is registered on the parent commit."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import DETECTORS, HEADS
    assert HEADS.get('AutoAssignHead') is detectors.AutoAssignHead and DETECTORS.get('AutoAssign') is detectors.AutoAssign


def test_config_builds_with_the_references_keys():
    from dsl_amd.detectors import FCOS, AutoAssign, AutoAssignHead
    m = build()
    assert isinstance(m, AutoAssign) and isinstance(m, FCOS) and isinstance(m.bbox_head, AutoAssignHead)
    o = m.store.head
    assert (o.head_kind, o.box_loss, o.bbox_weight, o.conv_bias, o.pos_loss_weight, o.neg_loss_weight, o.center_loss_weight) == \
        ('autoassign', 'giou', 5.0, True, 0.25, 0.75, 0.75)
    sd = m.state_dict()
    head = [k for k in sd if k.startswith('bbox_head.')]
    assert sorted(head) == sorted(str(k) for k in load_case('a')['d']['head_keys'])
    assert 'bbox_head.cls_convs.0.conv.bias' in sd                                     # conv_bias=True is forced (:151)
    assert sd['bbox_head.center_prior.mean'].shape == sd['bbox_head.center_prior.sigma'].shape == (80, 2)
    # autoassign_head.py:39-40 and :161-171
    assert not bool(sd['bbox_head.center_prior.mean'].any()) and bool((sd['bbox_head.center_prior.sigma'] == 1).all())
    assert float(sd['bbox_head.conv_cls.bias'][0]) == pytest.approx(-np.log(49.0), rel=1e-6)
    assert bool((sd['bbox_head.conv_reg.bias'] == 4.0).all()) and not bool(sd['bbox_head.conv_centerness.bias'].any())
    assert 0.008 < float(sd['bbox_head.conv_reg.weight'].std()) < 0.012
    m2 = build()
    m2.load_state_dict({k: v + 1 if v.dtype.is_floating_point else v for k, v in sd.items()})
    assert torch.equal(m2.state_dict()['bbox_head.center_prior.sigma'], sd['bbox_head.center_prior.sigma'] + 1)
    assert torch.equal(m2.state_dict()['bbox_head.center_prior.mean'], sd['bbox_head.center_prior.mean'] + 1)


def test_build_groups_places_the_prior():
    """configs/autoassign's optimizer: paramwise_cfg=dict(norm_decay_mult=0.).  The prior is neither bias nor norm: group 0, decayed,
    lr_mult 1; it lies in the head's gradient bucket and in the optimizer's bias mask as a weight."""
    from dsl_amd.optim import build_groups
    m = build()
    table, ids, by = build_groups(m, dict(norm_decay_mult=0.))
    assert table[0] == (1.0, 1.0) and by['bbox_head.center_prior.mean'] == by['bbox_head.center_prior.sigma'] == 0
    assert table[by['bbox_head.cls_convs.0.gn.weight']] == (1.0, 0.0)
    off, n, shape = m.store.train_regions['head.center_prior']
    assert shape == (2, 80, 2) and off + n == m.store.n_train and not bool(ids[off:off + n].any()) and not bool(m.store.group[off:off + n].any())
    lo, hi = m.store.grad_buckets()[0]
    assert lo <= off and off + n <= hi
    _, _, by2 = build_groups(m, dict(bias_lr_mult=2.0, bias_decay_mult=0.0))
    assert by2['bbox_head.center_prior.sigma'] == 0 and by2['bbox_head.conv_cls.bias'] != 0


BAD_HEADS = [(dict(force_topk=True), 'force_topk'), (dict(stacked_convs=3), 'stacked_convs'), (dict(norm_cfg=None), 'GN-32'),
             (dict(strides=[4, 8, 16, 32, 64]), 'strides'), (dict(loss_bbox=dict(type='DIoULoss')), 'GIoULoss'),
             (dict(loss_bbox=dict(type='IoULoss')), 'GIoULoss'), (dict(dcn_on_last_conv=True), 'DCN'), (dict(conv_bias=False), 'conv_bias'),
             (dict(center_sampling=True), 'center_sampling'), (dict(soft_weight=0.1), 'soft_weight'), (dict(pos_loss_weight=-1.0), 'pos_loss_weight')]


@pytest.mark.parametrize('head,what', BAD_HEADS, ids=[w + str(i) for i, (_, w) in enumerate(BAD_HEADS)])
def test_head_refusals(head, what):
    with pytest.raises(NotImplementedError, match=what):
        build(aa_model_cfg(**head))


def test_class_count_and_box_weight_are_refused_on_the_host():
    """The kernels' limits (1..128 classes: a lane owns two; a finite weight >= 0) are stated where the model is built, not first by
    the loss launch."""
    with pytest.raises(NotImplementedError, match='num_classes must be in 1..128'):
        build(aa_model_cfg(num_classes=129))
    for w in (-1.0, float('inf')):
        with pytest.raises(NotImplementedError, match='loss_weight'):
            build(aa_model_cfg(loss_bbox=dict(type='GIoULoss', loss_weight=w)))
    assert build(aa_model_cfg(num_classes=128)).store.num_classes == 128


def test_detector_wants_its_head_and_fcos_head_keeps_its_refusal():
    cfg = aa_model_cfg()
    cfg['bbox_head'] = fcos_model_cfg()['bbox_head']
    with pytest.raises(NotImplementedError, match='AutoAssignHead'):
        build(cfg)
    with pytest.raises(NotImplementedError, match='fp8'):
        build(dict(aa_model_cfg(), fp8=dict(layers='towers')))
    # GIoULoss(loss_weight=5.0) is accepted by AutoAssignHead (and ATSSHead); FCOSHead's own refusal stays
    cfg = fcos_model_cfg()
    cfg['bbox_head']['loss_bbox'] = dict(type='GIoULoss', loss_weight=5.0)
    with pytest.raises(NotImplementedError, match='loss_weight'):
        build(cfg)
