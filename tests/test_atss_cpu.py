"""ATSS without a GPU: tests/atss_ref.py against what the reference's own ATSSHead computed (tests/golden/atss_*.npz, written by
tests/golden/make_atss_golden.py), and the configuration surface of ATSSHead / ATSS / FPN(relu_before_extra_convs=False)."""
import copy

import pytest
import torch

import atss_ref as AR
from util import fcos_model_cfg

T = torch.from_numpy
CASES = 'abcdef'


def load_case(d):
    B, C = int(d['B']), int(d['num_classes'])
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    return dict(B=B, C=C, sizes=sizes, topk=int(d['topk']), anchor_scale=float(d['anchor_scale']), stds=tuple(float(v) for v in d['stds']),
                bbox_weight=float(d['bbox_weight']), pads=[tuple(int(v) for v in p) for p in d['pads']],
                gts=[T(d[f'gt{i}']) for i in range(B)], gls=[T(d[f'gl{i}']) for i in range(B)],
                cls=[T(d[f'cls{l}']) for l in range(5)], reg=[T(d[f'reg{l}']) for l in range(5)], ctr=[T(d[f'ctr{l}']) for l in range(5)],
                scales=T(d['scales']))


def ref_assign(c):
    return AR.assign(c['sizes'], c['gts'], c['gls'], c['pads'], c['topk'], c['anchor_scale'], c['C'])


def atss_model_cfg(**head):
    """Head, neck, train_cfg and test_cfg of configs/atss/atss_r50_fpn_1x_coco.py on the caffe ResNet-50 of configs/fcos."""
    cfg = fcos_model_cfg()
    cfg['type'] = 'ATSS'
    cfg['neck'] = dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs='on_output',
                       num_outs=5)
    bbox_head = dict(type='ATSSHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                     anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                           strides=[8, 16, 32, 64, 128]),
                     bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[0.1, 0.1, 0.2, 0.2]),
                     loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                     loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
                     loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))
    bbox_head.update(head)
    cfg['bbox_head'] = bbox_head
    cfg['train_cfg'] = dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False)
    cfg['test_cfg'] = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
    return cfg


def build(cfg=None):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(cfg or atss_model_cfg())


# ---- the model against the reference's outputs -----------------------------------------------------------------------------------
def test_fixture_covers_the_cases(golden):
    d = {c: golden(f'atss_{c}.npz') for c in CASES}
    assert all(int(d[c]['B']) == 2 and [tuple(s) for s in d[c]['sizes']] == AR.SIZES for c in CASES)
    assert 1 <= len(d['a']['gt0']) <= 40 and len(d['b']['gt1']) == 0 and int(d['b']['npos'][1]) == 0
    for i, k in ((0, 0), (1, 1)):           # d: a box whose centre lies within 4 px of the border
        b = d['d'][f'gt{i}'][0]
        assert (b[k] + b[k + 2]) / 2 < 4.0
    assert tuple(d['e']['pads'][1]) == (96, 128) and (int(d['f']['topk']), float(d['f']['anchor_scale'])) == (3, 4.0)
    # c: boxes share candidates - some anchor is a candidate of two boxes
    c = load_case(d['c'])
    seen = [set((l, i) for l, i, _, _ in cand) for cand in AR.assign_image(c['sizes'], c['gts'][0], c['gls'][0], c['pads'][0])[4]]
    assert any(seen[a] & seen[b] for a in range(len(seen)) for b in range(a))
    # e: invalid anchors on every level
    inv = [int((~m).sum()) for m in AR.valid_masks(AR.SIZES, (96, 128))]
    assert all(v > 0 for v in inv)
    assert (T(d['e']['cls_weight']) == 0).sum() == sum(inv)


@pytest.mark.parametrize('case', CASES)
def test_ref_assignment_equals_reference(golden, case):
    d = golden(f'atss_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    assert torch.equal(a['labels'], T(d['labels']).long())
    assert torch.equal(a['assign_idx'], T(d['assign_idx']).int())
    assert torch.equal(a['cls_weight'], T(d['cls_weight']).float())
    assert torch.equal(a['targets'], T(d['targets']))
    assert a['npos'] == [int(v) for v in d['npos']] and a['num_total'] == int(d['num_total'])


@pytest.mark.parametrize('case', CASES)
def test_ref_decode_and_losses_equal_reference(golden, case):
    """fp32 / float64 of the same formulas against the reference's fp32: rel 1e-5."""
    d = golden(f'atss_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    pos = T(d['pos']).long()
    assert torch.equal(pos, (a['labels'] < c['C']).nonzero().view(-1))
    anchors = AR.flat_anchors(c['sizes'], c['B'], c['anchor_scale'])
    assert torch.equal(anchors[pos], T(d['anchors_pos']))
    lvl = torch.cat([torch.full((c['B'] * h * w,), i) for i, (h, w) in enumerate(c['sizes'])])
    raw = AR.levels_to_flat(c['reg'])
    dec = AR.decode(anchors[pos], raw[pos] * c['scales'][lvl[pos]][:, None], c['stds'])
    assert torch.allclose(dec, T(d['decoded']), rtol=1e-5, atol=1e-5 * 160)
    # decode(encode(gt)) == gt up to rounding: the stored box is the reference's target
    assert torch.allclose(AR.decode(anchors[pos], T(d['deltas'])[pos], c['stds']), a['targets'][pos], rtol=1e-5, atol=1e-3)
    ct = AR.centerness_target(anchors[pos], a['targets'][pos])
    assert torch.allclose(ct, T(d['ctr_targets']), rtol=1e-4, atol=1e-6)
    cls, ctr = AR.levels_to_flat(c['cls']), AR.levels_to_flat(c['ctr'])[:, 0]
    lc, lb, lt, csum = AR.loss(cls, raw, ctr, c['scales'], a, c['sizes'], c['B'], c['C'], c['anchor_scale'], c['stds'], c['bbox_weight'])
    for got, k in ((lc, 'loss_cls'), (lb, 'loss_bbox'), (lt, 'loss_centerness')):
        assert float(got) == pytest.approx(float(d[k]), rel=1e-5), k
    assert csum == pytest.approx(float(d['ctr_sum']), rel=1e-5)


def test_ref_gradients_equal_reference(golden):
    d = golden('atss_a.npz')
    c = load_case(d)
    a = ref_assign(c)
    cls = AR.levels_to_flat(c['cls']).double().requires_grad_()
    raw = AR.levels_to_flat(c['reg']).double().requires_grad_()
    ctr = AR.levels_to_flat(c['ctr'])[:, 0].double().requires_grad_()
    sc = c['scales'].double().requires_grad_()
    lc, lb, lt, _ = AR.loss(cls, raw, ctr, sc, a, c['sizes'], c['B'], c['C'], c['anchor_scale'], c['stds'], c['bbox_weight'])
    (lc + lb + lt).backward()
    for got, k in ((cls.grad, 'gcls'), (raw.grad, 'greg')):
        want = AR.levels_to_flat([T(d[f'{k}{l}']) for l in range(5)]).double()
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-7 * float(want.abs().max()) + 1e-12), k
    assert torch.allclose(sc.grad, T(d['gscales']).double(), rtol=1e-4, atol=1e-7)
    # an active dw / dh clamp on a positive: no gradient through it
    pos = T(d['pos']).long()
    lvl = torch.cat([torch.full((c['B'] * h * w,), i) for i, (h, w) in enumerate(c['sizes'])])
    dwh = (raw.detach()[pos] * sc.detach()[lvl[pos]][:, None])[:, 2:] * torch.tensor(c['stds'][2:])
    act = dwh.abs() > AR.MAX_RATIO
    assert bool(act.any()) and float(raw.grad[pos][:, 2:][act].abs().max()) == 0.0


# ---- configuration surface ------------------------------------------------------------------------------------------------------
def test_atss_config_builds_on_the_caffe_backbone():
    from dsl_amd import _lib as L
    from dsl_amd.detectors import ATSS, ATSSHead
    m = build()
    assert isinstance(m, ATSS) and isinstance(m.bbox_head, ATSSHead)
    o = m.store.head
    assert (o.assigner, o.atss_topk, o.anchor_scale, o.delta_stds) == ('atss', 9, 8.0, (0.1, 0.1, 0.2, 0.2))
    assert (o.box_loss, o.bbox_weight, o.centerness_on_reg, o.conv_bias) == ('giou', 2.0, True, False)
    assert o.flags() == L.HEAD_ATSS | L.HEAD_LOSS_EXT and not o.is_default()
    assert m.store.fpn_relu_extra is False and m.neck.relu_before_extra_convs is False
    assert not [k for k in m.store.train_regions if k.endswith('.conv.bias') and 'bbox_head' in k]
    a = o.atss_desc()
    assert (a.topk, a.anchor_scale, list(a.delta_stds)) == (9, 8.0, pytest.approx([0.1, 0.1, 0.2, 0.2]))


def test_loss_plan_descriptor_of_an_atss_head():
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    o = HeadOptions(assigner='atss', atss_topk=3, anchor_scale=4.0, bbox_weight=2.0)
    p = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o, max_gt=64)
    assert p.desc.head_flags == L.HEAD_ATSS | L.HEAD_LOSS_EXT and p.desc.atss and p.desc.w_bbox == 2.0
    assert (p.atss.topk, p.atss.max_gt, p.atss.anchor_scale) == (3, 64, 4.0)
    with pytest.raises(ValueError, match='pad_shape'):
        p.set_targets([torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2)
    assert FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8))).atss is None


def _with(path, value):
    cfg = atss_model_cfg()
    node = cfg
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value
    return cfg


@pytest.mark.parametrize('path,value,word', [
    (('bbox_head', 'anchor_generator', 'ratios'), [0.5, 1.0, 2.0], 'ratios'),
    (('bbox_head', 'anchor_generator', 'scales_per_octave'), 3, 'scales_per_octave'),
    (('bbox_head', 'anchor_generator', 'octave_base_scale'), 0, 'octave_base_scale'),
    (('bbox_head', 'anchor_generator', 'strides'), [4, 8, 16, 32, 64], 'strides'),
    (('bbox_head', 'anchor_generator', 'type'), 'SSDAnchorGenerator', 'AnchorGenerator'),
    (('bbox_head', 'bbox_coder', 'type'), 'TBLRBBoxCoder', 'DeltaXYWHBBoxCoder'),
    (('bbox_head', 'bbox_coder', 'target_means'), [0.1, 0., 0., 0.], 'target_means'),
    (('bbox_head', 'bbox_coder', 'target_stds'), [0.1, 0.1, 0.0, 0.2], 'target_stds'),
    (('train_cfg', 'assigner', 'type'), 'MaxIoUAssigner', 'ATSSAssigner'),
    (('train_cfg', 'assigner', 'topk'), 17, 'topk'),
    (('train_cfg', 'assigner', 'ignore_iof_thr'), 0.5, 'ignore_iof_thr'),
    (('train_cfg', 'allowed_border'), 0, 'allowed_border'),
    (('train_cfg', 'pos_weight'), 2.0, 'pos_weight'),
    (('bbox_head', 'soft_weight'), 1.0, 'soft_weight'),
    (('bbox_head', 'loss_weight'), 3.0, 'loss_weight'),
    (('bbox_head', 'stacked_convs'), 2, 'stacked_convs'),
    (('bbox_head', 'reg_decoded_bbox'), True, 'reg_decoded_bbox'),
    (('bbox_head', 'loss_bbox'), dict(type='GIoULoss', loss_weight=-1.0), 'loss_weight'),
])
def test_refused_options_are_named(path, value, word):
    with pytest.raises(NotImplementedError, match=word):
        build(_with(path, value))


def test_fp8_towers_and_other_heads_stay_refused():
    from dsl_amd.registry import build_detector
    with pytest.raises(NotImplementedError, match='fp8 towers'):
        build_detector(dict(atss_model_cfg(), fp8=dict(layers='towers')))
    cfg = atss_model_cfg()
    cfg['bbox_head'] = fcos_model_cfg()['bbox_head']
    with pytest.raises(NotImplementedError, match='ATSSHead'):
        build_detector(cfg)


def test_existing_head_keys_are_unchanged():
    from dsl_amd.params import HeadOptions
    assert HeadOptions().key() == (True, True, True, False, True) and HeadOptions().flags() == 0
    assert HeadOptions(center_sampling=False, norm_on_bbox=False, centerness_on_reg=False, iou_loss=True, conv_bias=False).key() == \
        (False, False, False, True, False)
    assert HeadOptions(box_loss='diou', bbox_weight=2.0).key() == (True, True, True, False, True, 'diou', 1e-6, 2.0, 0.25, 1.0, 2.0, 1.0)
    k = HeadOptions(assigner='atss').key()
    assert k[:5] == (True, True, True, False, False) and k[5:] == ('atss', 9, 8.0, (0.1, 0.1, 0.2, 0.2))
    assert HeadOptions(assigner='atss', atss_topk=3).key() != k and HeadOptions(assigner='atss', bbox_weight=2.0).key()[-4:] == k[5:]
    with pytest.raises(NotImplementedError, match='assigner'):
        HeadOptions(assigner='max_iou')
    with pytest.raises(NotImplementedError, match='atss_topk'):
        HeadOptions(assigner='atss', atss_topk=0)


def test_state_dict_names_round_trip():
    m = build()
    sd = m.state_dict()
    names = ('bbox_head.atss_cls', 'bbox_head.atss_reg', 'bbox_head.atss_centerness')
    assert all(f'{n}.{leaf}' in sd for n in names for leaf in ('weight', 'bias'))
    assert not [k for k in sd if '.conv_cls.' in k or '.conv_reg.' in k or '.conv_centerness.' in k]
    assert [tuple(sd[f'{n}.weight'].shape) for n in names] == [(80, 256, 3, 3), (4, 256, 3, 3), (1, 256, 3, 3)]
    assert all(f'bbox_head.scales.{i}.scale' in sd for i in range(5)) and 'bbox_head.cls_convs.0.conv.bias' not in sd
    assert 'bbox_head.cls_convs.3.gn.weight' in sd and 'bbox_head.reg_convs.0.conv.weight' in sd
    # init (atss_head.py:30-42): Normal(0, 0.01) convolutions, the focal prior on atss_cls's bias
    assert float(sd['bbox_head.atss_cls.bias'][0]) == pytest.approx(-4.59511985, rel=1e-6) and float(sd['bbox_head.atss_reg.bias'].abs().max()) == 0
    assert 0.005 < float(sd['bbox_head.atss_cls.weight'].std()) < 0.02
    g = torch.Generator().manual_seed(5)
    new = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    m.load_state_dict(copy.deepcopy(new))
    out = m.state_dict()
    for k, v in new.items():
        assert torch.equal(out[k], v), k
    with pytest.raises(KeyError, match='conv_cls|atss_cls'):
        m.load_state_dict({k.replace('atss_cls', 'conv_cls'): v for k, v in new.items()})
