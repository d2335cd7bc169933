"""FCOSHead options off the fcos_semi "tricks" head, host side (no GPU): the reference's configs/fcos/ files build, the parameter store
follows conv_bias / centerness_on_reg, the refusals name what is built, and tests/head_options_ref.py - the restatement the GPU tests
compare against - reproduces the reference's own outputs (tests/golden/make_golden_head_options.py)."""
import os

import numpy as np
import pytest
import torch

import head_options_ref as HR
from util import fcos_model_cfg, levels_to_flat

T = torch.from_numpy
REF_DIR = '/root/reference/configs/fcos'
PLAIN_FILES = ['fcos_r50_caffe_fpn_gn-head_1x_coco.py', 'fcos_r50_caffe_fpn_gn-head_4x4_1x_coco.py',
               'fcos_r50_caffe_fpn_gn-head_mstrain_640-800_2x_coco.py', 'fcos_center_r50_caffe_fpn_gn-head_1x_coco.py']
LOSS_LEGS = ['loss_opt_centerness_on_reg_c18', 'loss_plain_sup', 'loss_plain_sup_ig', 'loss_plain_dsl', 'loss_plain_nopos', 'loss_opt_center_sampling',
             'loss_opt_norm_on_bbox', 'loss_opt_centerness_on_reg', 'loss_opt_iou_loss', 'loss_opt_conv_bias']
PLAIN_HEAD = dict(center_sampling=False, norm_on_bbox=False, centerness_on_reg=False, conv_bias='auto',
                  loss_bbox=dict(type='IoULoss', loss_weight=1.0))


def build(**head):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    return build_detector(fcos_model_cfg(**head))


def opts_of(d):
    return {k: bool(int(d[k])) for k in HR.DEFAULT}


@pytest.mark.skipif(not os.path.exists(REF_DIR), reason='reference tree not present')
@pytest.mark.parametrize('name', PLAIN_FILES)
def test_reference_fcos_configs_build_unmodified(name):
    from dsl_amd import detectors, runner  # noqa: F401
    from dsl_amd.optim import build_optimizer
    from dsl_amd.registry import Config, build_detector
    cfg = Config.fromfile(os.path.join(REF_DIR, name))
    m = build_detector(cfg.model)
    o = m.bbox_head.options
    center = name.startswith('fcos_center')
    assert o.key() == (center, False, False, True, False), o
    assert m.store.head is o and not m.store.convs['bbox_head.cls_convs.0.conv'].bias
    # _base_ inheritance: the schedule's SGD settings under this file's lr / paramwise_cfg, grad_clip replacing the inherited None
    assert cfg.optimizer.type == 'SGD' and cfg.optimizer.lr == 0.01 and cfg.optimizer.momentum == 0.9
    opt = build_optimizer(m, cfg.optimizer, grad_clip=cfg.optimizer_config.get('grad_clip'))
    assert opt.max_norm == 35.0 and opt.bias_lr_mult == 2.0 and opt.bias_decay_mult == 0.0
    assert cfg.runner.max_epochs == (24 if 'mstrain' in name else 12) and cfg.data.samples_per_gpu == (4 if '4x4' in name else 2)


@pytest.mark.parametrize('conv_bias', [True, False])
def test_state_dict_keys_follow_conv_bias_and_round_trip(golden, conv_bias):
    """Key set == the reference model's (net_tiny_plain.npz stores the plain model's; with biases: the 377 keys of the tricks model);
    load -> state_dict returns the values; a dictionary of the other kind is refused."""
    sd = HR.plain_state_dict(0, conv_bias=conv_bias)
    m = build(**dict(PLAIN_HEAD, conv_bias=conv_bias))
    out = m.state_dict()
    assert set(out) == set(sd) and len(out) == (377 if conv_bias else 369)
    if not conv_bias:
        assert sorted(out) == [str(k) for k in golden('net_tiny_plain.npz')['state_keys']]
        assert not [k for k in out if HR.is_tower_bias(k)]
        assert not [k for k in m.store.train_regions if k.endswith('.conv.bias') and 'bbox_head' in k]
    m.load_state_dict(sd)
    out = m.state_dict()
    for k, v in sd.items():
        assert tuple(out[k].shape) == tuple(v.shape) and torch.equal(out[k], v), k
    assert sorted(k for k, p in m.named_parameters() if p.requires_grad) == sorted(HR.trainable_keys(sd))
    # conv_centerness lives with the classification predictor (centerness_on_reg=False): row round_up(C, 4), rows between stay zero
    st = m.store
    assert st.ctr_on_cls and torch.equal(st.tview('head.cls_w')[80].permute(2, 0, 1), sd['bbox_head.conv_centerness.weight'][0])
    assert float(st.tview('head.cls_w')[81:].abs().max()) == 0 and float(st.tview('head.regctr_w')[4:].abs().max()) == 0
    other = HR.plain_state_dict(0, conv_bias=not conv_bias)
    with pytest.raises(KeyError, match='conv.bias'):
        m.load_state_dict(other)
    # the gradient buckets still tile the flat buffer, and only real bias regions are in the optimizer's bias group
    lo_hi = st.grad_buckets()
    assert lo_hi[-1][0] == 0 and lo_hi[0][1] == st.n_train and all(a[0] == b[1] for a, b in zip(lo_hi[:-1], lo_hi[1:]))
    nb = sum(n for k, (off, n, shape) in st.train_regions.items() if k.endswith('.conv.bias') or k in ('head.cls_b', 'head.regctr_b'))
    assert int(st.group.sum()) == nb


def test_default_head_layout_is_unchanged():
    m = build()
    st = m.store
    assert st.head.is_default() and st.head.flags() == 0 and not st.ctr_on_cls
    assert (st.cls_pad, st.cls_ld, st.logit_ld, st.cls_rows) == (128, 80, 80, 80) and len(m.state_dict()) == 377


def test_refusals_name_what_is_built():
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_loss
    for kw, word in ((dict(linear=True), 'linear'), (dict(eps=1e-7), 'eps'), (dict(mode='linear'), 'mode'), (dict(loss_weight=2.0), 'loss_weight')):
        with pytest.raises(NotImplementedError, match=word):
            build_loss(dict(type='IoULoss', **kw))
    for kw, word in ((dict(dcn_on_last_conv=True), 'DCN'), (dict(stacked_convs=2), 'stacked_convs=4'),
                     (dict(loss_bbox=dict(type='GIoULoss', loss_weight=2.0)), 'loss_weight'), (dict(conv_bias='yes'), 'conv_bias')):
        with pytest.raises(NotImplementedError, match=word):
            build(**kw)
    cfg = fcos_model_cfg()
    cfg['backbone']['depth'] = 101
    from dsl_amd.registry import build_detector
    with pytest.raises(NotImplementedError, match='ResNet-50'):
        build_detector(cfg)
    cfg = fcos_model_cfg()
    cfg['backbone']['type'] = 'ResNeXt'
    with pytest.raises(KeyError, match='ResNeXt'):
        build_detector(cfg)
    # fp8 towers: the default head only, by name
    with pytest.raises(NotImplementedError, match='fp8 towers'):
        build_detector(dict(fcos_model_cfg(**PLAIN_HEAD), fp8=dict(layers='towers')))
    assert build_detector(dict(fcos_model_cfg(), fp8=dict(layers='towers'))).store.fp8
    # the centerness column needs room behind the classes
    with pytest.raises(NotImplementedError, match='num_classes <= 124'):
        build(num_classes=126, centerness_on_reg=False)
    assert build(num_classes=124, centerness_on_reg=False).store.cls_pad == 128
    assert build(num_classes=64, centerness_on_reg=False).store.cls_pad == 128


# ---- the restatement against the reference's own outputs ----------------------------------------------------------------------
@pytest.mark.parametrize('name', ['assign_plain_small.npz', 'assign_plain_full.npz'])
def test_ref_assignment_identical_to_reference(golden, name):
    from oracle import fcos_oracle as O
    d = golden(name)
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    n = int(d['n_img'])
    gtb, gtl = [T(d[f'gt{i}']) for i in range(n)], [T(d[f'gl{i}']) for i in range(n)]
    for norm, key in ((False, 'bbox_targets_t'), (True, 'bbox_targets_norm_t')):
        labels, tg, _ = HR.get_targets(O.get_points(sizes), gtb, gtl, HR.options(center_sampling=False, norm_on_bbox=norm))
        assert torch.equal(torch.cat(labels), T(d['labels']).long())
        assert torch.equal(torch.cat(tg), T(d[key]).t())
    # inside-box differs from centre sampling on these boxes (the fixture is not vacuous)
    lab_cs = torch.cat(HR.get_targets(O.get_points(sizes), gtb, gtl, HR.DEFAULT)[0])
    assert int((lab_cs != T(d['labels']).long()).sum()) > 0


def load_loss_leg(d):
    B = int(d['B'])
    leg = dict(B=B, sizes=[tuple(int(v) for v in s) for s in d['sizes']], opts=opts_of(d),
               gtb=[T(d[f'gt{i}']) for i in range(B)], gtl=[T(d[f'gl{i}']) for i in range(B)],
               ig=[T(d[f'ig{i}']) for i in range(B)] if int(d['with_ig']) else None,
               cls=[T(d[f'cls{i}']) for i in range(5)], reg=[T(d[f'reg{i}']) for i in range(5)], ctr=[T(d[f'ctr{i}']) for i in range(5)],
               scales=T(d['scales']), loss_weight=float(d['loss_weight']), soft_weight=float(d['soft_weight']),
               C=int(d['num_classes']))
    return leg


@pytest.mark.parametrize('name', LOSS_LEGS)
def test_ref_loss_matches_reference_to_fp32_rounding(golden, name):
    d = golden(name + '.npz')
    leg = load_loss_leg(d)
    assert int(d['num_pos']) >= 20 or name.endswith('nopos')
    o = leg['opts']
    cls = [c.clone().requires_grad_() for c in leg['cls']]
    reg = [r.clone().requires_grad_() for r in leg['reg']]
    ctr = [c.clone().requires_grad_() for c in leg['ctr']]
    sc = leg['scales'].clone().requires_grad_()
    pred = [torch.relu(r * sc[i]) if o['norm_on_bbox'] else (r * sc[i]).exp() for i, r in enumerate(reg)]
    out = HR.fcos_loss(cls, pred, ctr, leg['gtb'], leg['gtl'], leg['ig'], opts=o, loss_weight=leg['loss_weight'],
                       soft_weight=leg['soft_weight'], soft_scale=1e-3, num_classes=leg['C'])        # (generated inside the warm-up window)
    sum(out.values()).backward()
    for k in ('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft'):
        if k in d.files:
            assert float(out[k]) == pytest.approx(float(d[k]), rel=2e-6, abs=1e-7), k
    for mine, key in ((cls, 'gcls'), (reg, 'greg'), (ctr, 'gctr')):
        for i in range(5):
            ref = T(d[f'{key}{i}'])
            g = mine[i].grad if mine[i].grad is not None else torch.zeros_like(ref)
            assert torch.allclose(g, ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()) + 1e-12), (key, i)
    assert torch.allclose(sc.grad, T(d['gscales']), rtol=1e-5, atol=1e-7)


def test_ref_whole_model_matches_reference(golden):
    d = golden('net_tiny_plain.npz')
    sd = HR.plain_state_dict(0)
    B = int(d['B'])
    gtb, gtl = [T(d[f'gt{i}']) for i in range(B)], [T(d[f'gl{i}']) for i in range(B)]
    losses, grads, aux = HR.train_step(sd, T(d['img']), gtb, gtl, None, opts=HR.PLAIN)
    for k in ('loss_cls', 'loss_bbox', 'loss_centerness'):
        assert losses[k] == pytest.approx(float(d[k]), rel=1e-4), k
    for i in range(5):
        for key in ('cls', 'reg', 'ctr'):
            assert torch.allclose(aux[key][i].detach(), T(d[f'{key}{i}']), rtol=1e-3, atol=1e-4), (key, i)
    keys = [str(k) for k in d['grad_keys']]
    assert sorted(keys) == sorted(grads)
    for k, n in zip(keys, d['grad_norms']):
        assert float(grads[k].norm()) == pytest.approx(float(n), rel=2e-3, abs=1e-6), k
    for k in d.files:
        if k.startswith('grad/'):
            ref = T(d[k])
            assert torch.allclose(grads[k[5:]], ref, rtol=1e-2, atol=2e-3 * float(ref.abs().max()) + 1e-9), k
