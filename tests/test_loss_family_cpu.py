"""The configurable FCOS losses, host side (no GPU): tests/loss_family_ref.py - the restatement the GPU tests compare against -
reproduces the reference's own outputs (tests/golden/make_golden_loss_family.py), the configuration surface builds what is built
and refuses the rest by name, and every edge case of tests/test_loss_family_gpu.py is well conditioned: the restatement in float32
agrees with itself in float64 within that test's bars."""
import numpy as np
import pytest
import torch

import head_options_ref as HR
import loss_family_ref as LR
from test_head_options_cpu import PLAIN_HEAD, build, load_loss_leg
from util import fcos_model_cfg, levels_to_flat

T = torch.from_numpy
FAM_LEGS = ['loss_fam_diou', 'loss_fam_ciou', 'loss_fam_ciou_dsl_c18', 'loss_fam_iou_linear', 'loss_fam_focal_all', 'loss_fam_focal_g0',
            'loss_fam_focal_g3']
LOSS_KEYS = ('box_loss', 'box_eps', 'focal_gamma', 'focal_alpha', 'cls_weight', 'bbox_weight', 'ctr_weight')
POW2_SCALES = (1.0, 0.5, 2.0, 1.0, 0.25)


def load_fam_leg(d):
    """load_loss_leg plus the fixture's loss settings (the default ones for a fixture from before the loss family)."""
    leg = load_loss_leg(d)
    leg['loss'] = LR.loss_settings()
    if 'box_loss' in d.files:
        leg['loss'] = {k: (str(d[k]) if k == 'box_loss' else float(d[k])) for k in LOSS_KEYS}
    return leg


def split_levels(flat, leg, c):
    B = leg['B']
    return [t.view(B, h, w, c).permute(0, 3, 1, 2) for t, (h, w) in zip(flat.split([B * h * w for h, w in leg['sizes']]), leg['sizes'])]


def ref_run(leg, dtype=torch.float32, raw=None, cls=None, soft_scale=1e-3):
    """The restatement on a leg's operands in `dtype` (the targets are the float32 assignment's in either case): losses, and the
    gradients w.r.t. the raw regression output, the Scale parameters, the class and the centerness logits, flat [M][.]."""
    o = leg['opts']
    raw = (levels_to_flat(leg['reg']) if raw is None else raw).to(dtype).clone().requires_grad_()
    cls = (levels_to_flat(leg['cls']) if cls is None else cls).to(dtype).clone().requires_grad_()
    ctr = levels_to_flat(leg['ctr']).to(dtype).clone().requires_grad_()
    sc = leg['scales'].to(dtype).clone().requires_grad_()
    z = [r * sc[i] for i, r in enumerate(split_levels(raw, leg, 4))]
    pred = [torch.relu(t) if o['norm_on_bbox'] else t.exp() for t in z]
    out = LR.fcos_loss(split_levels(cls, leg, leg['C']), pred, split_levels(ctr, leg, 1), leg['gtb'], leg['gtl'], leg['ig'], opts=o,
                       loss=leg['loss'], loss_weight=leg['loss_weight'], soft_weight=leg['soft_weight'], soft_scale=soft_scale,
                       num_classes=leg['C'])
    sum(out.values()).backward()
    zero = torch.zeros_like
    grads = dict(reg=raw.grad if raw.grad is not None else zero(raw), cls=cls.grad, ctr=(ctr.grad if ctr.grad is not None else zero(ctr))[:, 0],
                 scales=sc.grad if sc.grad is not None else zero(sc))
    return {k: float(v.detach()) for k, v in out.items()}, grads


# ---- 1. the restatement against the reference's own outputs ------------------------------------------------------------------
@pytest.mark.parametrize('name', FAM_LEGS)
def test_ref_loss_family_matches_reference_to_fp32_rounding(golden, name):
    """The bars of test_head_options_cpu.test_ref_loss_matches_reference_to_fp32_rounding."""
    d = golden(name + '.npz')
    leg = load_fam_leg(d)
    assert int(d['num_pos']) >= 20
    out, g = ref_run(leg)
    for k in ('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft'):
        if k in d.files:
            assert out[k] == pytest.approx(float(d[k]), rel=2e-6, abs=1e-7), k
    assert ('loss_sisoft' in d.files) == (name == 'loss_fam_ciou_dsl_c18')
    for key, fix in (('cls', 'gcls'), ('reg', 'greg'), ('ctr', 'gctr')):
        ref = levels_to_flat([T(d[f'{fix}{i}']) for i in range(5)])
        ref = ref[:, 0] if key == 'ctr' else ref
        assert torch.isfinite(ref).all()
        assert torch.allclose(g[key], ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()) + 1e-12), key
    assert torch.allclose(g['scales'], T(d['gscales']), rtol=1e-5, atol=1e-7)


def test_fixture_legs_cover_the_family(golden):
    legs = {n: load_fam_leg(golden(n + '.npz')) for n in FAM_LEGS}
    want = dict(loss_fam_diou=('diou', True, 80, 2.0), loss_fam_ciou=('ciou', False, 80, 0.5), loss_fam_ciou_dsl_c18=('ciou', True, 18, 1.0),
                loss_fam_iou_linear=('iou_linear', False, 80, 1.0))
    for n, (kind, relu, C, wb) in want.items():
        leg = legs[n]
        assert (leg['loss']['box_loss'], leg['opts']['norm_on_bbox'], leg['C'], leg['loss']['bbox_weight']) == (kind, relu, C, wb), n
    dsl = legs['loss_fam_ciou_dsl_c18']
    assert dsl['B'] == 3 and dsl['loss_weight'] == 3.0 and dsl['soft_weight'] == 1.0 and not dsl['opts']['centerness_on_reg'] and dsl['ig']
    assert not legs['loss_fam_iou_linear']['opts']['center_sampling']
    fa = legs['loss_fam_focal_all']['loss']
    assert (fa['focal_gamma'], fa['focal_alpha'], fa['cls_weight'], fa['bbox_weight'], fa['ctr_weight'], fa['box_loss']) == (1.5, 0.5, 0.25, 1.5, 2.0, 'giou')
    assert (legs['loss_fam_focal_g0']['loss']['focal_gamma'], legs['loss_fam_focal_g0']['loss']['focal_alpha']) == (0.0, 0.75)
    assert legs['loss_fam_focal_g3']['loss']['focal_gamma'] == 3.0


# ---- 2. the configuration surface -----------------------------------------------------------------------------------------------
FOCAL = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
CTR = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)


@pytest.mark.parametrize('head,want', [
    (dict(loss_bbox=dict(type='DIoULoss', loss_weight=2.0)), dict(box_loss='diou', bbox_weight=2.0, box_eps=1e-6)),
    (dict(loss_bbox=dict(type='CIoULoss', eps=1e-5, reduction='mean', loss_weight=0.5)), dict(box_loss='ciou', bbox_weight=0.5, box_eps=1e-5)),
    (dict(loss_bbox=dict(type='CIoULoss'), loss_cls=dict(FOCAL, gamma=3.0), loss_centerness=dict(CTR, loss_weight=0.5)),
     dict(box_loss='ciou', bbox_weight=1.0, focal_gamma=3.0, ctr_weight=0.5, iou_loss=False)),
    (dict(loss_cls=dict(FOCAL, gamma=1.5, alpha=0.5, loss_weight=0.25)), dict(focal_gamma=1.5, focal_alpha=0.5, cls_weight=0.25)),
    (dict(loss_cls=dict(FOCAL, gamma=0.0, alpha=1.0)), dict(focal_gamma=0.0, focal_alpha=1.0)),
    (dict(loss_centerness=dict(CTR, loss_weight=2.0)), dict(ctr_weight=2.0)),
    (dict(loss_cls=dict(FOCAL, loss_weight=0.0)), dict(cls_weight=0.0)),
])
def test_new_loss_configs_build_and_reach_the_descriptor(head, want):
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    m = build(**head)
    o = m.bbox_head.options
    assert m.store.head is o and not o.is_default() and not o.loss_is_default() and o.flags() & L.HEAD_LOSS_EXT
    for k, v in want.items():
        assert getattr(o, k) == v, (k, getattr(o, k))
    assert o.key()[:5] == (True, True, True, o.iou_loss, True) and o.key()[5:] == o.loss_key() and len(o.key()) == 12 and 'box_loss' in repr(o)
    # the parameter layout does not depend on the losses: they own no parameters
    assert len(m.state_dict()) == 377 and m.store.n_train == build().store.n_train
    d = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o).desc
    assert d.head_flags == o.flags() and d.box_kind == HeadOptions.BOX_KINDS[o.box_loss]
    got = (d.box_eps, d.focal_gamma, d.focal_alpha, d.w_cls, d.w_bbox, d.w_ctr)
    assert got == pytest.approx((o.box_eps, o.focal_gamma, o.focal_alpha, o.cls_weight, o.bbox_weight, o.ctr_weight), rel=1e-7)
    # fp8 towers stay with the default head
    from dsl_amd.registry import build_detector
    with pytest.raises(NotImplementedError, match='fp8 towers'):
        build_detector(dict(fcos_model_cfg(**head), fp8=dict(layers='towers')))


def test_old_configs_keep_their_key_flags_and_descriptor():
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    assert HeadOptions().key() == (True, True, True, False, True) and HeadOptions().flags() == 0 and HeadOptions().is_default()
    for cs in (False, True):
        for nb in (False, True):
            for cr in (False, True):
                for iou in (False, True):
                    for cb in (False, True):
                        o = HeadOptions(cs, nb, cr, iou, cb)
                        assert o.key() == (cs, nb, cr, iou, cb) and o.loss_is_default()
                        assert o.flags() == ((0 if cs else 1) | (0 if nb else 6) | (8 if iou else 0))
                        assert o.is_default() == ((cs, nb, cr, iou, cb) == (True, True, True, False, True))
                        assert repr(o) == f'HeadOptions(center_sampling={cs}, norm_on_bbox={nb}, centerness_on_reg={cr}, iou_loss={iou}, conv_bias={cb})'
    # explicit default loss settings are the default head; the descriptor's new fields stay zero
    o = HeadOptions(box_loss='giou', focal_gamma=2, focal_alpha=0.25, cls_weight=1, bbox_weight=1, ctr_weight=1)
    assert o.is_default() and o.flags() == 0
    assert HeadOptions(box_loss='iou').key() == HeadOptions(iou_loss=True).key() == (True, True, True, True, True)
    for head in (None, HeadOptions(), HeadOptions(False, False, False, True, False)):
        d = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=head).desc
        assert not d.head_flags & L.HEAD_LOSS_EXT
        assert (d.box_kind, d.box_eps, d.focal_gamma, d.focal_alpha, d.w_cls, d.w_bbox, d.w_ctr) == (0, 0, 0, 0, 0, 0, 0)
    m, p = build(), build(**PLAIN_HEAD)
    assert m.bbox_head.options.key() == (True, True, True, False, True) and p.bbox_head.options.key() == (False, False, False, True, False)
    assert m.bbox_head.options.flags() == 0 and p.bbox_head.options.flags() == 15
    with pytest.raises(NotImplementedError, match='box_loss'):
        HeadOptions(box_loss='bounded')


@pytest.mark.parametrize('cfg,word', [
    (dict(type='FocalLoss', reduction='sum'), 'reduction'), (dict(type='DIoULoss', reduction='none'), 'reduction'),
    (dict(type='CIoULoss', reduction='sum'), 'reduction'), (dict(type='IoULoss', reduction='sum'), 'reduction'),
    (dict(type='GIoULoss', reduction='sum'), 'reduction'), (dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='sum'), 'reduction'),
    (dict(type='FocalLoss', use_sigmoid=False), 'use_sigmoid'), (dict(type='FocalLoss', gamma=-0.5), 'gamma'),
    (dict(type='FocalLoss', alpha=1.5), 'alpha'), (dict(type='FocalLoss', alpha=-0.1), 'alpha'),
    (dict(type='BoundedIoULoss', beta=0.2), 'broadcast'), (dict(type='GIoULoss', loss_weight=-1.0), 'loss_weight'),
    (dict(type='CIoULoss', loss_weight=float('nan')), 'loss_weight'), (dict(type='DIoULoss', eps=0.0), 'eps'),
    (dict(type='IoULoss', eps=1e-7), 'eps'), (dict(type='IoULoss', mode='linear'), 'mode'),
    # pinned by test_head_options_cpu.test_refusals_name_what_is_built: the config classes keep these; HeadOptions runs them (below)
    (dict(type='IoULoss', linear=True), 'linear'), (dict(type='IoULoss', loss_weight=2.0), 'loss_weight'),
    (dict(type='GIoULoss', loss_weight=2.0), 'loss_weight'),
])
def test_rejected_loss_configs_name_the_reason(cfg, word):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_loss
    with pytest.raises(NotImplementedError, match=word):
        build_loss(cfg)


@pytest.mark.parametrize('kw,kind,ext', [(dict(box_loss='iou_linear'), 2, True), (dict(box_loss='iou', bbox_weight=3.0), 1, True),
                                         (dict(box_loss='giou', bbox_weight=1.5), 0, True), (dict(iou_loss=True, bbox_weight=0.0), 1, True),
                                         (dict(box_loss='iou'), 1, False)])
def test_head_options_carry_the_box_kinds_the_config_classes_refuse(kw, kind, ext):
    """Linear IoU and a weighted GIoU / IoU-log loss through params.HeadOptions -> FcosLossPlan -> descriptor."""
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    from dsl_amd.params import HeadOptions
    o = HeadOptions(**kw)
    assert o.iou_loss == (kind in (1, 2)) and bool(o.flags() & L.HEAD_LOSS_EXT) == ext == (len(o.key()) == 12) and o.is_default() is False
    assert bool(o.flags() & L.HEAD_IOU_LOSS) == (kind == 1)
    d = FcosLossPlan(2, [(4, 6), (2, 3)], 'cpu', strides=(8, 16), ranges=((-1, 64), (64, 1e8)), head=o).desc
    assert d.head_flags == o.flags()
    if ext:
        assert d.box_kind == kind and d.w_bbox == pytest.approx(o.bbox_weight) and (d.focal_gamma, d.focal_alpha, d.w_cls, d.w_ctr) == (2.0, 0.25, 1.0, 1.0)


def test_unknown_loss_type_and_wrong_role_are_refused():
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_loss
    with pytest.raises(KeyError, match='EIoULoss'):
        build_loss(dict(type='EIoULoss'))
    with pytest.raises(NotImplementedError, match='CIoULoss'):
        build(loss_bbox=dict(type='FocalLoss'))
    with pytest.raises(NotImplementedError, match='CIoULoss'):
        build(loss_cls=dict(type='CIoULoss'))


# ---- 3. the GPU test's edge cases: float32 against float64 on the restatement ---------------------------------------------------
NEW_KINDS = ('iou_linear', 'diou', 'ciou')
EDGE_CASES = ([('coincide', k) for k in ('diou', 'ciou')] + [(c, k) for c in ('zero_lr', 'zero_tb', 'zero_all') for k in NEW_KINDS]
              + [('linear_clamp', 'iou_linear')] + [('no_positives', k) for k in NEW_KINDS] + [('saturated', g) for g in (0.0, 0.5, 1.5)]
              + [('weight0', w) for w in ('cls_weight', 'bbox_weight', 'ctr_weight')])
N_EDGE = 8        # locations (or logits per sign) that a case rewrites


def edge_case(golden, case, arg):
    """(leg, raw regression output [M][4], class logits [M][C], rewritten positive rows) of an edge case.  Base legs: relu decode ->
    loss_fam_diou, exp decode + inside-box assignment -> loss_fam_iou_linear, no positives -> loss_plain_nopos,
    focal -> loss_fam_focal_all."""
    from oracle import fcos_oracle as O
    base = dict(linear_clamp='loss_fam_iou_linear', no_positives='loss_plain_nopos', saturated='loss_fam_focal_all',
                weight0='loss_fam_focal_all').get(case, 'loss_fam_diou')
    leg = load_fam_leg(golden(base + '.npz'))
    if case == 'saturated':
        leg['loss'] = dict(leg['loss'], focal_gamma=arg)
    elif case == 'weight0':
        leg['loss'] = dict(leg['loss'], **{arg: 0.0})
    else:
        leg['loss'] = LR.loss_settings(box_loss=arg, bbox_weight=1.0)
    labels, tg, _ = HR.get_targets(O.get_points(leg['sizes']), leg['gtb'], leg['gtl'], leg['opts'], leg['C'])
    fl, ft = torch.cat(labels), torch.cat(tg)
    lvl = torch.cat([torch.full((leg['B'] * h * w,), i) for i, (h, w) in enumerate(leg['sizes'])])
    pos = (fl < leg['C']).nonzero().view(-1)
    raw, cls = levels_to_flat(leg['reg']).clone(), levels_to_flat(leg['cls']).clone()
    rows = pos[:N_EDGE]
    assert len(rows) == (0 if case == 'no_positives' else N_EDGE)
    if case == 'coincide':         # relu decode with power-of-two scales: raw * scale == target, bit for bit
        leg['scales'] = torch.tensor(POW2_SCALES)
        raw[rows] = ft[rows] / leg['scales'][lvl[rows]].view(-1, 1)
        assert torch.equal(torch.relu(raw[rows] * leg['scales'][lvl[rows]].view(-1, 1)), ft[rows]) and leg['opts']['norm_on_bbox']
    if case.startswith('zero'):    # the relu gate closed on left + right, top + bottom, or all four sides
        cols = dict(zero_lr=[0, 2], zero_tb=[1, 3], zero_all=[0, 1, 2, 3])[case]
        for c in cols:
            raw[rows, c] = -1.0
        assert leg['opts']['norm_on_bbox']
    if case == 'linear_clamp':     # exp(14 * scale): boxes of 10^4 .. 10^7 pixels, iou < 1e-6
        raw[rows] = 14.0
        assert not leg['opts']['norm_on_bbox']
    if case == 'saturated':        # +-40 on the label's logit of positive rows and on background logits
        neg = (fl == leg['C']).nonzero().view(-1)
        for k in range(N_EDGE):
            cls[rows[k], fl[rows[k]]] = 40.0 if k % 2 else -40.0
            cls[neg[k], (7 * k) % leg['C']] = 40.0 if k % 2 else -40.0
    return leg, raw, cls, rows


def within_gpu_bars(l_a, g_a, l_b, g_b):
    """The GPU test's bars, `a` measured against `b`."""
    for k in l_b:
        assert l_a[k] == pytest.approx(l_b[k], rel=1e-4, abs=1e-6), (k, l_a[k], l_b[k])
    for key in ('cls', 'reg', 'ctr'):
        a, b = g_a[key].float(), g_b[key].float()
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), key
        assert torch.allclose(a, b, rtol=2 ** -7, atol=2 ** -8 * float(b.abs().max()) * 0.05 + 1e-9), key
    assert torch.allclose(g_a['scales'].float(), g_b['scales'].float(), rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize('case,arg', EDGE_CASES)
def test_edge_cases_are_well_conditioned_fp32_vs_fp64(golden, case, arg):
    leg, raw, cls, rows = edge_case(golden, case, arg)
    l32, g32 = ref_run(leg, torch.float32, raw, cls)
    l64, g64 = ref_run(leg, torch.float64, raw, cls)
    within_gpu_bars(l32, g32, l64, g64)
    if case == 'linear_clamp':
        assert float(g64['reg'][rows].abs().max()) == 0.0 and float(g32['reg'][rows].abs().max()) == 0.0
    if case == 'no_positives':
        assert l64['loss_bbox'] == 0.0 and float(g64['reg'].abs().max()) == 0.0
    if case == 'weight0':
        key = dict(cls_weight='cls', bbox_weight='reg', ctr_weight='ctr')[arg]
        assert float(g64[key].abs().max()) == 0.0 and l64['loss_' + dict(cls='cls', reg='bbox', ctr='centerness')[key]] == 0.0


def test_reference_is_nan_where_the_two_deviations_apply():
    """What the deviations replace: autograd through the reference's formulas gives NaN for CIoU at coincident boxes (float32) and
    for gamma < 1 at a saturated sigmoid; the restatement gives the float64 value / the limit."""
    import math
    box = torch.tensor([[10., 20., 50., 90.]])
    p = box.clone().requires_grad_()
    eps = 1e-6
    ov = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    iou = ov / (ov + ov.detach() - ov + eps)
    v = 4 / math.pi ** 2 * (torch.atan((box[:, 2] - box[:, 0]) / (box[:, 3] - box[:, 1] + eps)) - torch.atan((p[:, 2] - p[:, 0]) / (p[:, 3] - p[:, 1] + eps))) ** 2
    assert torch.isnan(v ** 2 / (1 - iou + v)).all()
    mine = LR.box_loss_elem('ciou', p, box, eps)
    mine.sum().backward()
    assert torch.isfinite(mine).all() and torch.isfinite(p.grad).all()
    assert float(mine) == pytest.approx(float(LR.box_loss_elem('ciou', box.double(), box.double(), eps)), abs=1e-6)
    x = torch.tensor([[40.0]], requires_grad=True)
    pt = 1 - x.sigmoid()
    (pt.pow(0.5) * torch.nn.functional.binary_cross_entropy_with_logits(x, torch.ones(1, 1), reduction='none')).sum().backward()
    assert torch.isnan(x.grad).all()
    y = torch.tensor([[40.0]], requires_grad=True)
    LR.focal_loss_elem(y, torch.tensor([0]), 1, gamma=0.5, alpha=0.25).sum().backward()
    assert float(y.grad) == pytest.approx(0.0, abs=1e-12)
