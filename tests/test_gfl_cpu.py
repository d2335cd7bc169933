"""GFL without a GPU: tests/gfl_ref.py against what the reference's own GFLHead computed (tests/golden/gfl_*.npz, written by
tests/golden/make_gfl_golden.py), the configuration surface of GFLHead / GFL, the parameter layout of a GFL head and the unchanged
keys / offsets of every head that existed before."""
import copy

import pytest
import torch

import atss_ref as AR
import gfl_ref as GR
from test_atss_cpu import atss_model_cfg
from util import fcos_model_cfg

T = torch.from_numpy
CASES = 'abcdef'
BOX_KINDS = dict(GIoULoss='giou', DIoULoss='diou')


def load_case(d):
    B, C = int(d['B']), int(d['num_classes'])
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    return dict(B=B, C=C, sizes=sizes, topk=int(d['topk']), anchor_scale=float(d['anchor_scale']), reg_max=int(d['reg_max']),
                beta=float(d['beta']), cls_weight=float(d['cls_weight']), bbox_weight=float(d['bbox_weight']), dfl_weight=float(d['dfl_weight']),
                box_kind=BOX_KINDS[str(d['box_kind'])], pads=[tuple(int(v) for v in p) for p in d['pads']],
                gts=[T(d[f'gt{i}']) for i in range(B)], gls=[T(d[f'gl{i}']) for i in range(B)],
                cls=[T(d[f'cls{l}']) for l in range(5)], reg=[T(d[f'reg{l}']) for l in range(5)], scales=T(d['scales']))


def ref_assign(c):
    return AR.assign(c['sizes'], c['gts'], c['gls'], c['pads'], c['topk'], c['anchor_scale'], c['C'])


def loss_kw(c):
    return dict(num_classes=c['C'], reg_max=c['reg_max'], beta=c['beta'], cls_weight=c['cls_weight'], bbox_weight=c['bbox_weight'],
                dfl_weight=c['dfl_weight'], box_kind=c['box_kind'])


def gfl_model_cfg(**head):
    """Head, neck, train_cfg and test_cfg of configs/gfl/gfl_r50_fpn_1x_coco.py on the caffe ResNet-50 of configs/fcos."""
    cfg = atss_model_cfg()
    cfg['type'] = 'GFL'
    bbox_head = dict(type='GFLHead', num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
                     anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                           strides=[8, 16, 32, 64, 128]),
                     loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0),
                     loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25), reg_max=16,
                     loss_bbox=dict(type='GIoULoss', loss_weight=2.0))
    bbox_head.update(head)
    cfg['bbox_head'] = bbox_head
    return cfg


def build(cfg=None):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(cfg or gfl_model_cfg())


# ---- the model against the reference's outputs -----------------------------------------------------------------------------------
def test_fixture_covers_the_cases(golden):
    d = {c: golden(f'gfl_{c}.npz') for c in CASES}
    assert all(int(d[c]['B']) == 2 and [tuple(s) for s in d[c]['sizes']] == AR.SIZES for c in CASES)
    assert (int(d['a']['num_classes']), int(d['a']['reg_max'])) == (80, 16) and 1 <= len(d['a']['gt0']) <= 40
    assert all(int(d[c]['num_classes']) == 3 for c in 'bcdef')
    assert len(d['b']['gt1']) == 0 and int(d['b']['npos'][1]) == 0 and int(d['b']['npos'][0]) > 0
    assert int(d['c']['reg_max']) == 15 and d['c']['reg0'].shape[1] == 64
    assert int(d['d']['reg_max']) == 3
    hit = T(d['d']['dfl_targets']) == T(d['d']['dfl_targets']).max()          # clamped at reg_max - 0.1, and some are not
    assert float(T(d['d']['dfl_targets']).max()) == pytest.approx(2.9, rel=1e-6) and bool(hit.any()) and not bool(hit.all())
    assert tuple(d['e']['pads'][1]) == (96, 128)
    assert (float(d['f']['beta']), float(d['f']['dfl_weight']), str(d['f']['box_kind'])) == (1.5, 0.5, 'DIoULoss')


@pytest.mark.parametrize('case', CASES)
def test_ref_assignment_equals_reference(golden, case):
    d = golden(f'gfl_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    assert torch.equal(a['labels'], T(d['labels']).long()) and torch.equal(a['assign_idx'], T(d['assign_idx']).int())
    assert torch.equal(a['cls_weight'], T(d['cls_weight_map']).float()) and torch.equal(a['targets'], T(d['targets']))
    assert a['npos'] == [int(v) for v in d['npos']] and a['num_total'] == int(d['num_total'])


@pytest.mark.parametrize('case', CASES)
def test_ref_decode_quality_and_losses_equal_reference(golden, case):
    """fp32 / float64 of the same formulas against the reference's fp32: rel 1e-5 (test_atss_cpu's bars)."""
    d = golden(f'gfl_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    cls, raw = AR.levels_to_flat(c['cls']), AR.levels_to_flat(c['reg'])
    pos, pred, tgt, ctr, _, _ = GR.decode_pos(raw, c['scales'], a, c['sizes'], c['B'], c['reg_max'], c['C'])
    assert torch.equal(pos, T(d['pos']).long())
    assert torch.allclose(pred, T(d['decoded']), rtol=1e-5, atol=1e-5 * 20) and torch.allclose(tgt, T(d['tgt']), rtol=1e-6, atol=0)
    assert torch.allclose(GR.dfl_targets(ctr, tgt, c['reg_max']), T(d['dfl_targets']), rtol=1e-6, atol=1e-6)
    score, weight, wsum = GR.quality(cls, raw, c['scales'], a, c['sizes'], c['B'], c['reg_max'], c['C'])
    assert torch.allclose(score[pos], T(d['score']), rtol=1e-4, atol=1e-6) and torch.allclose(weight[pos], T(d['weight']), rtol=1e-5, atol=0)
    assert float(wsum) == pytest.approx(float(d['weight_sum']), rel=1e-5)
    off = torch.ones(len(score), dtype=torch.bool)
    off[pos] = False
    assert float(score[off].abs().max()) == 0.0 and float(weight[off].abs().max()) == 0.0
    lc, lb, ld, _ = GR.loss(cls.double(), raw.double(), c['scales'].double(), a, c['sizes'], c['B'], **loss_kw(c))
    for got, k in ((lc, 'loss_cls'), (lb, 'loss_bbox'), (ld, 'loss_dfl')):
        assert float(got) == pytest.approx(float(d[k]), rel=1e-5), k


@pytest.mark.parametrize('case', CASES)
def test_ref_gradients_equal_reference(golden, case):
    d = golden(f'gfl_{case}.npz')
    c = load_case(d)
    a = ref_assign(c)
    cls = AR.levels_to_flat(c['cls']).double().requires_grad_()
    raw = AR.levels_to_flat(c['reg']).double().requires_grad_()
    sc = c['scales'].double().requires_grad_()
    lc, lb, ld, _ = GR.loss(cls, raw, sc, a, c['sizes'], c['B'], **loss_kw(c))
    (lc + lb + ld).backward()
    for got, k in ((cls.grad, 'gcls'), (raw.grad, 'greg')):
        want = AR.levels_to_flat([T(d[f'{k}{l}']) for l in range(5)]).double()
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-7 * float(want.abs().max()) + 1e-12), k
    assert torch.allclose(sc.grad, T(d['gscales']).double(), rtol=1e-4, atol=1e-7)
    off = (a['labels'] >= c['C']).nonzero().view(-1)
    assert float(raw.grad[off].abs().max()) == 0.0


def test_no_box_at_all_has_unit_normalisers(golden):
    c = load_case(golden('gfl_b.npz'))
    c['gts'], c['gls'] = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    a = ref_assign(c)
    cls, raw = AR.levels_to_flat(c['cls']).double(), AR.levels_to_flat(c['reg']).double()
    lc, lb, ld, (score, weight, wsum) = GR.loss(cls, raw, c['scales'].double(), a, c['sizes'], c['B'], **loss_kw(c))
    assert a['num_total'] == 2 and float(wsum) == 0.0 and float(lb) == 0.0 and float(ld) == 0.0 and float(lc) > 0


# ---- configuration surface ------------------------------------------------------------------------------------------------------
def test_gfl_config_builds_on_the_caffe_backbone():
    from dsl_amd import _lib as L
    from dsl_amd.detectors import GFL, DistributionFocalLoss, GFLHead, QualityFocalLoss
    m = build()
    assert isinstance(m, GFL) and isinstance(m.bbox_head, GFLHead)
    assert isinstance(m.bbox_head.loss_cls, QualityFocalLoss) and isinstance(m.bbox_head.loss_dfl, DistributionFocalLoss)
    o = m.store.head
    assert (o.head_kind, o.reg_max, o.qfl_beta, o.dfl_weight) == ('gfl', 16, 2.0, 0.25)
    assert (o.assigner, o.atss_topk, o.anchor_scale, o.box_loss, o.bbox_weight, o.cls_weight, o.conv_bias) == ('atss', 9, 8.0, 'giou', 2.0, 1.0, False)
    assert o.flags() == L.HEAD_ATSS | L.HEAD_LOSS_EXT | L.HEAD_GFL and not o.is_default()
    assert m.store.fpn_relu_extra is False
    assert not [k for k in m.store.train_regions if k.endswith('.conv.bias') and 'bbox_head' in k]
    f = build(gfl_model_cfg(reg_max=7, loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=1.5, loss_weight=0.5),
                            loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.5), loss_bbox=dict(type='DIoULoss', loss_weight=1.5)))
    o = f.store.head
    assert (o.reg_max, o.qfl_beta, o.dfl_weight, o.cls_weight, o.box_loss, o.bbox_weight) == (7, 1.5, 0.5, 0.5, 'diou', 1.5)


def test_loss_plan_descriptor_of_a_gfl_head():
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    o = HeadOptions(head_kind='gfl', reg_max=16, bbox_weight=2.0, qfl_beta=1.5, dfl_weight=0.5)
    p = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o, max_gt=64, num_classes=3)
    g = p.gfl
    assert g.fcos.head_flags == L.HEAD_ATSS | L.HEAD_LOSS_EXT | L.HEAD_GFL and g.fcos.atss and g.fcos.w_bbox == 2.0 and g.fcos.num_classes == 3
    assert (g.reg_max, g.qfl_beta, g.w_dfl) == (16, 1.5, 0.5) and g.score and g.weight
    assert (p.LD_RC, p.LD_GRC, g.fcos.ld_rc, g.fcos.ld_grc) == (68, 128, 68, 128) and tuple(p.g_rc.shape) == (p.M, 128)
    assert not g.fcos.ctr and not g.fcos.g_ctr and len(p.logvec) == 4
    q = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=HeadOptions(head_kind='gfl', reg_max=15))
    assert (q.LD_RC, q.LD_GRC) == (64, 64)
    # a GFL head with the default loss family carries its loss settings too: dsl_gfl_loss reads them with no default to fall back to
    for plan_, kind in ((q, L.BOX_GIOU), (FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)),
                                                      head=HeadOptions(head_kind='gfl', box_loss='iou')), L.BOX_IOU_LOG)):
        f = plan_.gfl.fcos
        assert (f.w_cls, f.w_bbox, f.box_kind, f.focal_gamma, f.focal_alpha) == (1.0, 1.0, kind, 2.0, 0.25) and f.head_flags & L.HEAD_LOSS_EXT
        assert (plan_.gfl.qfl_beta, plan_.gfl.w_dfl) == (2.0, 0.25)
    plain = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)))
    assert plain.gfl is None and (plain.LD_RC, plain.LD_GRC) == (8, 64)


def _with(path, value):
    cfg = gfl_model_cfg()
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
    (('train_cfg', 'assigner', 'type'), 'MaxIoUAssigner', 'ATSSAssigner'),
    (('train_cfg', 'assigner', 'topk'), 17, 'topk'),
    (('train_cfg', 'allowed_border'), 0, 'allowed_border'),
    (('bbox_head', 'norm_cfg'), dict(type='BN'), 'norm_cfg'),
    (('bbox_head', 'stacked_convs'), 2, 'stacked_convs'),
    (('bbox_head', 'feat_channels'), 128, 'feat_channels'),
    (('bbox_head', 'conv_cfg'), dict(type='DCNv2'), 'conv_cfg'),
    (('bbox_head', 'reg_max'), 17, r'reg_max in 1\.\.16'),
    (('bbox_head', 'reg_max'), 0, r'reg_max in 1\.\.16'),
    (('bbox_head', 'loss_cls'), dict(type='FocalLoss', use_sigmoid=True), 'QualityFocalLoss'),
    (('bbox_head', 'loss_cls'), dict(type='QualityFocalLoss', use_sigmoid=False), 'use_sigmoid'),
    (('bbox_head', 'loss_cls'), dict(type='QualityFocalLoss', beta=-1.0), 'beta'),
    (('bbox_head', 'loss_dfl'), dict(type='CrossEntropyLoss', use_sigmoid=True), 'DistributionFocalLoss'),
    (('bbox_head', 'loss_dfl'), dict(type='DistributionFocalLoss', loss_weight=-0.25), 'loss_weight'),
    (('bbox_head', 'loss_bbox'), dict(type='GIoULoss', loss_weight=-1.0), 'loss_weight'),
    (('bbox_head', 'soft_weight'), 1.0, 'soft_weight'),
    (('bbox_head', 'soft_warm_up'), 100, 'soft_warm_up'),
    (('bbox_head', 'loss_weight'), 3.0, 'loss_weight'),
])
def test_refused_options_are_named(path, value, word):
    with pytest.raises(NotImplementedError, match=word):
        build(_with(path, value))


def test_fp8_towers_and_other_heads_stay_refused():
    from dsl_amd.params import HeadOptions
    from dsl_amd.registry import build_detector
    with pytest.raises(NotImplementedError, match='fp8 towers'):
        build_detector(dict(gfl_model_cfg(), fp8=dict(layers='towers')))
    cfg = gfl_model_cfg()
    cfg['bbox_head'] = atss_model_cfg()['bbox_head']
    with pytest.raises(NotImplementedError, match='GFLHead'):
        build_detector(cfg)
    with pytest.raises(NotImplementedError, match=r'reg_max must be an integer in 1\.\.16'):
        HeadOptions(head_kind='gfl', reg_max=17)
    with pytest.raises(NotImplementedError, match='head_kind'):
        HeadOptions(head_kind='ld')
    for kw, word in ((dict(centerness_on_reg=False), 'centerness_on_reg'), (dict(norm_on_bbox=False), 'norm_on_bbox'),
                     (dict(center_sampling=False), 'center_sampling'), (dict(iou_loss=True), 'iou_loss'), (dict(focal_gamma=1.5), 'focal_gamma'),
                     (dict(focal_alpha=0.5), 'focal_alpha'), (dict(ctr_weight=2.0), 'ctr_weight'), (dict(assigner='max_iou'), 'assigner')):
        with pytest.raises(NotImplementedError, match=word):
            HeadOptions(head_kind='gfl', **kw)


# ---- parameter layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reg_max,rows,pad', [(15, 64, 64), (16, 68, 128), (3, 16, 64)])
def test_param_store_of_a_gfl_head(reg_max, rows, pad):
    from dsl_amd.params import HeadOptions, ParamStore
    st = ParamStore(3, head=HeadOptions(head_kind='gfl', reg_max=reg_max)).init_reference_style(1)
    assert (st.reg_rows, st.reg_pad, st.reg_ld) == (rows, pad, rows)
    assert st.train_regions['head.regctr_w'][2] == (pad, 3, 3, 256) and st.train_regions['head.regctr_b'][2] == (pad,)
    w, b = st.tview('head.regctr_w'), st.tview('head.regctr_b')
    assert float(w[:rows].std()) > 0.005 and bool((w[:rows].reshape(rows, -1).abs().max(1)[0] > 0).all())          # every real row is initialised
    if pad > rows:
        assert float(w[rows:].abs().max()) == 0.0 and float(b[rows:].abs().max()) == 0.0          # padding rows stay zero
    lay, _ = st.wT_layout()
    assert lay['head.regctr'][1] == 256 * 9 * pad
    sd = st.named_views()
    assert tuple(sd['bbox_head.gfl_reg.weight'].shape) == (rows, 256, 3, 3) and tuple(sd['bbox_head.gfl_cls.weight'].shape) == (3, 256, 3, 3)
    assert not [k for k in sd if 'centerness' in k or 'atss_' in k or '.conv_cls.' in k or '.conv_reg.' in k]
    assert st.grad_buckets()[0][1] == st.n_train


def test_state_dict_names_round_trip():
    m = build()
    sd = m.state_dict()
    names = ('bbox_head.gfl_cls', 'bbox_head.gfl_reg')
    assert all(f'{n}.{leaf}' in sd for n in names for leaf in ('weight', 'bias'))
    assert [tuple(sd[f'{n}.weight'].shape) for n in names] == [(80, 256, 3, 3), (68, 256, 3, 3)]
    assert all(f'bbox_head.scales.{i}.scale' in sd for i in range(5)) and 'bbox_head.cls_convs.0.conv.bias' not in sd
    assert not [k for k in sd if 'centerness' in k or 'atss_' in k or '.conv_cls.' in k]
    # init (gfl_head.py:73-82): Normal(0, 0.01) convolutions, the 0.01 prior on gfl_cls's bias
    assert float(sd['bbox_head.gfl_cls.bias'][0]) == pytest.approx(-4.59511985, rel=1e-6) and float(sd['bbox_head.gfl_reg.bias'].abs().max()) == 0
    assert 0.005 < float(sd['bbox_head.gfl_reg.weight'].std()) < 0.02
    g = torch.Generator().manual_seed(5)
    new = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    m.load_state_dict(copy.deepcopy(new))
    out = m.state_dict()
    for k, v in new.items():
        assert torch.equal(out[k], v), k
    assert float(m.store.tview('head.regctr_w')[68:].abs().max()) == 0.0
    with pytest.raises(KeyError, match='atss_cls|gfl_cls'):
        m.load_state_dict({k.replace('gfl_cls', 'atss_cls'): v for k, v in new.items()})


# ---- what existed before stays what it was ---------------------------------------------------------------------------------------
def test_existing_head_keys_are_unchanged():
    from dsl_amd.params import HeadOptions
    assert HeadOptions().key() == (True, True, True, False, True) and HeadOptions().flags() == 0
    assert HeadOptions(box_loss='diou', bbox_weight=2.0).key() == (True, True, True, False, True, 'diou', 1e-6, 2.0, 0.25, 1.0, 2.0, 1.0)
    assert HeadOptions(assigner='atss').key() == (True, True, True, False, False, 'atss', 9, 8.0, (0.1, 0.1, 0.2, 0.2))
    assert HeadOptions(assigner='atss', bbox_weight=2.0).key() == \
        (True, True, True, False, False, 'giou', 1e-6, 2.0, 0.25, 1.0, 2.0, 1.0, 'atss', 9, 8.0, (0.1, 0.1, 0.2, 0.2))
    assert HeadOptions(assigner='atss').flags() == 32 and repr(HeadOptions()).count('=') == 5
    k = HeadOptions(head_kind='gfl').key()
    assert k[-4:] == ('gfl', 16, 2.0, 0.25) and HeadOptions(head_kind='gfl', reg_max=15).key() != k


def test_default_param_store_offsets_are_the_parents():
    """Offsets of the flat training buffer for ParamStore(head=None), literals recorded from the commit before GFL."""
    from dsl_amd.params import HeadOptions, ParamStore
    st = ParamStore(80)
    got = {k: st.train_regions[k][0] for k in ('head.cls_w', 'head.cls_b', 'head.regctr_w', 'head.regctr_b', 'head.scales')}
    assert got == {'head.cls_w': 31825920, 'head.cls_b': 32120832, 'head.regctr_w': 32120960, 'head.regctr_b': 32268416, 'head.scales': 32268480}
    assert st.n_train == 32268488 and st.train_regions['head.regctr_w'][2] == (64, 3, 3, 256)
    assert (st.reg_rows, st.reg_pad, st.reg_ld) == (5, 64, 8) and st.predictor_names() == ('conv_cls', 'conv_reg', 'conv_centerness')
    a = ParamStore(80, head=HeadOptions(assigner='atss'))
    assert (a.reg_rows, a.reg_pad, a.reg_ld) == (5, 64, 8) and a.predictor_names() == ('atss_cls', 'atss_reg', 'atss_centerness')
    assert a.train_regions['head.regctr_w'][2] == (64, 3, 3, 256)
    o = ParamStore(80, head=HeadOptions(centerness_on_reg=False))
    assert (o.reg_rows, o.reg_pad, o.reg_ld) == (4, 64, 8)
