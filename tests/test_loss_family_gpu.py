"""The configurable FCOS losses on the GPU: DIoU / CIoU / linear IoU, focal gamma / alpha and the three loss weights - the loss launch
against the reference's own outputs (tests/golden/make_golden_loss_family.py) and, at the edges, against tests/loss_family_ref.py
in float64 (pinned to the reference, and checked for conditioning, by tests/test_loss_family_cpu.py); the default path bit for bit;
the whole step and a train_detector run with weighted losses."""
import json
import os

import numpy as np
import pytest
import torch

import head_options_ref as HR
import loss_family_ref as LR
from test_head_options_cpu import PLAIN_HEAD
from test_loss_family_cpu import EDGE_CASES, FAM_LEGS, edge_case, load_fam_leg, ref_run, within_gpu_bars
from util import fcos_model_cfg, levels_to_flat, oracle_threads, rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def head_options(leg, **loss):
    from dsl_amd.params import HeadOptions
    o = leg['opts']
    return HeadOptions(**{k: bool(o[k]) for k in HeadOptions.FIELDS}, **dict(leg['loss'], **loss))


def run_leg(leg, raw=None, cls=None, force_ext=False, **loss):
    """test_head_options_gpu.run_leg with the leg's loss settings: assign + loss in the engine's layout, NaN in the logits' padding
    columns.  force_ext: the descriptor carries the settings and HEAD_LOSS_EXT even where they are the default ones."""
    from dsl_amd import _lib as L
    from dsl_amd.head_loss import FcosLossPlan
    C = leg['C']
    head = head_options(leg, **loss)
    plan = FcosLossPlan(leg['B'], leg['sizes'], 'cuda', num_classes=C, head=head)
    if force_ext:
        head.fill_loss_desc(plan.desc)
        plan.desc.head_flags |= L.HEAD_LOSS_EXT
    plan.set_targets(leg['gtb'], leg['gtl'], leg['ig'])
    plan.configure(loss_weight=leg['loss_weight'], soft_weight=leg['soft_weight'] / 1000.0)
    plan.assign()
    M = plan.M
    logits = torch.full((M, plan.LD_CLS), float('nan'))
    logits[:, :C] = levels_to_flat(leg['cls']) if cls is None else cls
    rc = torch.zeros(M, 8)
    rc[:, :4] = levels_to_flat(leg['reg']) if raw is None else raw
    if plan.ctr_col is None:
        rc[:, 4] = levels_to_flat(leg['ctr'])[:, 0]
    else:
        logits[:, plan.ctr_col] = levels_to_flat(leg['ctr'])[:, 0]
        rc[:, 4] = float('nan')
    plan.bind_outputs(logits.cuda(), rc.cuda(), leg['scales'].cuda())
    plan.loss()
    torch.cuda.synchronize()
    return plan


def outputs(plan, C):
    """(losses by name, gradients by kind) of a finished plan, on the host."""
    got = plan.losses.cpu()
    losses = dict(loss_cls=float(got[0]), loss_bbox=float(got[1]), loss_centerness=float(got[2]))
    if plan.desc.soft_weight != 0.0:
        losses['loss_sisoft'] = float(got[3])
    ctr = (plan.g_rc[:, 4] if plan.ctr_col is None else plan.g_cls[:, plan.ctr_col]).float().cpu()
    return losses, dict(cls=plan.g_cls.float().cpu()[:, :C], reg=plan.g_rc.float().cpu()[:, :4], ctr=ctr, scales=plan.g_scales.cpu())


def same_bits(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ('losses', 'g_cls', 'g_rc', 'g_scales', 'logvec'))


@pytest.mark.parametrize('name', FAM_LEGS)
def test_loss_family_vs_reference_golden(golden, name):
    """The bars of test_head_options_gpu.test_loss_vs_reference_golden: loss sums rel 1e-4 / abs 1e-6, bf16 gradients 2^-8 with the same
    absolute term, g_scales rtol 1e-3, padding columns exactly 0, a second run bit-identical."""
    d = golden(name + '.npz')
    leg = load_fam_leg(d)
    plan = run_leg(leg)
    got = plan.losses.cpu()
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft')):
        if k in d.files:
            print(name, k, float(got[i]), float(d[k]))
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft')):
        if k in d.files:
            assert float(got[i]) == pytest.approx(float(d[k]), rel=1e-4, abs=1e-6), k
    # the log vector: the weighted terms in log order and their sum
    terms = [float(d[k]) for k in ('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft') if k in d.files]
    lv = plan.logvec.cpu()[:len(terms) + 1].tolist()
    assert lv == pytest.approx(terms + [sum(terms)], rel=1e-4, abs=1e-6)
    gc = levels_to_flat([T(d[f'gcls{i}']) for i in range(5)])
    gr = levels_to_flat([T(d[f'greg{i}']) for i in range(5)])
    gt_ = levels_to_flat([T(d[f'gctr{i}']) for i in range(5)])[:, 0]
    tol = 2 ** -8
    C = leg['C']
    _, g = outputs(plan, C)
    assert torch.allclose(g['cls'], gc, rtol=tol, atol=tol * float(gc.abs().max()) * 0.05 + 1e-9)
    assert torch.allclose(g['reg'], gr, rtol=tol, atol=tol * float(gr.abs().max()) * 0.05 + 1e-9)
    assert torch.allclose(g['ctr'], gt_, rtol=tol, atol=tol * float(gt_.abs().max()) * 0.05 + 1e-9)
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    if plan.ctr_col is None:
        assert float(mine_c[:, C:].abs().max()) == 0.0 and float(mine_r[:, 5:].abs().max()) == 0.0
    else:       # classes | zeros up to round_up(C, 4) | centerness | zeros
        assert plan.ctr_col == (C + 3) // 4 * 4 and float(mine_c[:, C:plan.ctr_col].abs().sum()) == 0.0
        assert float(mine_c[:, plan.ctr_col + 1:].abs().max()) == 0.0 and float(mine_r[:, 4:].abs().max()) == 0.0
    assert torch.allclose(g['scales'], T(d['gscales']), rtol=1e-3, atol=1e-6)
    assert same_bits(plan, run_leg(leg))


@pytest.mark.parametrize('case,arg', [c for c in EDGE_CASES if c[0] != 'weight0'])
def test_loss_family_edges_vs_fp64(golden, case, arg):
    """The pattern of test_head_options_gpu.test_iou_loss_edges_vs_fp64 on the new kinds: prediction bit-equal to its target (CIoU:
    finite, the float64 value), zero-width / zero-size predictions, the linear IoU loss with its clamp active (loss 1 - eps, gradient
    exactly 0), no positives, saturated logits with gamma 0 / 0.5 / 1.5 (finite, the limit) - against the restatement in float64."""
    leg, raw, cls, rows = edge_case(golden, case, arg)
    plan = run_leg(leg, raw, cls)
    l64, g64 = ref_run(leg, torch.float64, raw, cls)
    lg, gg = outputs(plan, leg['C'])
    print(case, arg, lg, l64)
    assert torch.isfinite(plan.g_cls.float()).all() and torch.isfinite(plan.g_rc.float()).all() and torch.isfinite(plan.g_scales).all()
    assert torch.isfinite(plan.losses).all()
    within_gpu_bars(lg, gg, l64, g64)
    if case == 'linear_clamp':
        assert float(gg['reg'][rows].abs().max()) == 0.0
    if case == 'no_positives':
        assert lg['loss_bbox'] == 0.0 and lg['loss_centerness'] == 0.0 and float(gg['reg'].abs().max()) == 0.0 and int(plan.stats[0]) == 0
        assert float(gg['ctr'].abs().max()) == 0.0 and float(gg['scales'].abs().max()) == 0.0


@pytest.mark.parametrize('which', ['cls_weight', 'bbox_weight', 'ctr_weight'])
def test_weight_zero_silences_one_term_and_leaves_the_others_bit_identical(golden, which):
    leg = load_fam_leg(golden('loss_fam_focal_all.npz'))
    C = leg['C']
    full, zero = run_leg(leg), run_leg(leg, **{which: 0.0})
    (lf, gf), (lz, gz) = outputs(full, C), outputs(zero, C)
    term = dict(cls_weight=('loss_cls', ['cls']), bbox_weight=('loss_bbox', ['reg', 'scales']), ctr_weight=('loss_centerness', ['ctr']))[which]
    assert lz[term[0]] == 0.0 and lf[term[0]] > 0.0
    for k in ('cls', 'reg', 'scales', 'ctr'):
        if k in term[1]:
            assert float(gz[k].abs().max()) == 0.0 and float(gf[k].abs().max()) > 0.0, k
        else:
            assert torch.equal(gz[k], gf[k]), k
    for k in lf:
        assert k == term[0] or lz[k] == lf[k], k
    assert float(zero.logvec[3]) == pytest.approx(sum(lz.values()), rel=1e-6)
    # 64-bit restatement of the silenced configuration
    l64, g64 = ref_run(dict(leg, loss=dict(leg['loss'], **{which: 0.0})), torch.float64)
    within_gpu_bars(lz, gz, l64, g64)


@pytest.mark.parametrize('name', ['loss_dsl.npz', 'loss_plain_sup.npz'])
def test_default_path_bits_do_not_depend_on_how_the_defaults_are_given(golden, name):
    """A descriptor whose new fields are zero and one that states gamma 2, alpha 0.25, unit weights and GIoU / IoU-log explicitly give
    the same bits, which meet the golden expectations the existing tests hold for these fixtures; with one term re-weighted (the
    family's kernel, gamma == 2 and GIoU / IoU-log inside it) the other terms' bits are still the default kernel's."""
    d = golden(name)
    if 'center_sampling' in d.files:
        leg = load_fam_leg(d)
    else:          # a fixture of the tricks head from before the head options: `reg` is bbox_pred itself (>= 0), so unit scales
        B = int(d['B'])
        leg = dict(B=B, sizes=[tuple(int(v) for v in s) for s in d['sizes']], opts=dict(HR.DEFAULT), C=80, loss=LR.loss_settings(),
                   gtb=[T(d[f'gt{i}']) for i in range(B)], gtl=[T(d[f'gl{i}']) for i in range(B)], ig=[T(d[f'ig{i}']) for i in range(B)],
                   cls=[T(d[f'cls{i}']) for i in range(5)], reg=[T(d[f'reg{i}']) for i in range(5)], ctr=[T(d[f'ctr{i}']) for i in range(5)],
                   scales=torch.ones(5), loss_weight=float(d['loss_weight']), soft_weight=float(d['soft_weight']))
        assert int(d['with_ig']) == 1 and int(d['soft_warm_up']) == 0
    C = leg['C']
    zero_fields = run_leg(leg)
    explicit = run_leg(leg, force_ext=True)
    from dsl_amd import _lib as L
    assert not zero_fields.desc.head_flags & L.HEAD_LOSS_EXT and zero_fields.desc.w_cls == 0.0
    assert explicit.desc.head_flags & L.HEAD_LOSS_EXT and (explicit.desc.focal_gamma, explicit.desc.w_cls) == (2.0, 1.0)
    assert same_bits(zero_fields, explicit)
    got = zero_fields.losses.cpu()
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft')):
        if k in d.files:
            assert float(got[i]) == pytest.approx(float(d[k]), rel=1e-4, abs=1e-6), k
    gc = levels_to_flat([T(d[f'gcls{i}']) for i in range(5)])
    tol = 2 ** -8
    assert torch.allclose(zero_fields.g_cls.float().cpu()[:, :C], gc, rtol=tol, atol=tol * float(gc.abs().max()) * 0.05 + 1e-9)
    half_ctr = run_leg(leg, ctr_weight=0.5)
    (l0, g0), (l1, g1) = outputs(zero_fields, C), outputs(half_ctr, C)
    assert torch.equal(g0['cls'], g1['cls']) and torch.equal(g0['reg'], g1['reg']) and torch.equal(g0['scales'], g1['scales'])
    assert l0['loss_cls'] == l1['loss_cls'] and l0['loss_bbox'] == l1['loss_bbox'] and l1['loss_centerness'] == 0.5 * l0['loss_centerness']
    half_box = run_leg(leg, bbox_weight=0.5)
    l2, g2 = outputs(half_box, C)
    assert torch.equal(g0['cls'], g2['cls']) and torch.equal(g0['ctr'], g2['ctr']) and l2['loss_bbox'] == 0.5 * l0['loss_bbox']


# ---- the whole step ---------------------------------------------------------------------------------------------------------
STEP_LOSS = dict(loss_bbox=dict(type='CIoULoss', loss_weight=2.0),
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.5, loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=0.5))
STEP_SETTINGS = dict(box_loss='ciou', box_eps=1e-6, focal_gamma=1.5, focal_alpha=0.5, cls_weight=1.0, bbox_weight=2.0, ctr_weight=0.5)


def test_train_step_and_train_detector_with_weighted_losses(golden, tmp_path):
    """The plain head at net_tiny_plain's size with CIoU (loss_weight 2), FocalLoss(gamma 1.5, alpha 0.5) and centerness weight 0.5:
    losses and parameter gradients against loss_family_ref.train_step by the noise model and bars of
    test_head_options_gpu.test_plain_train_step_vs_reference_and_restatement (no reference fixture of this combination exists: the
    float32 restatement, pinned to the reference per loss, stands in); then two iterations of train_detector from a config file
    written here, whose first logged losses are the weighted ones of that same batch."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config, build_detector
    d = golden('net_tiny_plain.npz')
    B = int(d['B'])
    model_cfg = fcos_model_cfg(**dict(PLAIN_HEAD, **STEP_LOSS))
    sd = HR.plain_state_dict(0)
    model = build_detector(model_cfg)
    model.load_state_dict(sd)
    model = model.cuda()
    o = model.bbox_head.options
    assert o.loss_key() == tuple(STEP_SETTINGS[k] for k in o.LOSS_FIELDS) and o.key()[:5] == (False, False, False, False, False)
    img = T(d['img'])
    gtb, gtl = [T(d[f'gt{i}']) for i in range(B)], [T(d[f'gl{i}']) for i in range(B)]
    metas = [dict(img_shape=tuple(img.shape[2:]) + (3,), pad_shape=tuple(img.shape[2:]) + (3,), scale_factor=1.0)] * B

    def step():
        model.store.grad.zero_()
        losses = model.forward_train(img.cuda(), metas, gtb, gtl)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        return {k: float(v.detach()) for k, v in losses.items()}, model.store.grad.clone()
    got, grad = step()
    opts = dict(HR.PLAIN, iou_loss=False)
    with oracle_threads():
        lem, gem, aux = LR.train_step(sd, img, gtb, gtl, None, opts=opts, loss=STEP_SETTINGS, emulate_bf16=True)
        l32, g32, aux32 = LR.train_step(sd, img, gtb, gtl, None, opts=opts, loss=STEP_SETTINGS, emulate_bf16=False)
    # the weights are in the restatement's terms: against the unit-weight CIoU run of the same operands
    unit, _ = LR.fcos_loss([t.detach() for t in aux32['cls']], [t.detach() for t in aux32['reg']], [t.detach() for t in aux32['ctr']], gtb, gtl,
                           None, opts=opts, loss=dict(STEP_SETTINGS, bbox_weight=1.0, ctr_weight=1.0), return_aux=True)
    assert l32['loss_bbox'] == pytest.approx(2.0 * float(unit['loss_bbox']), rel=1e-6)
    assert l32['loss_centerness'] == pytest.approx(0.5 * float(unit['loss_centerness']), rel=1e-6)
    for k in got:
        e_emu, e_hip = abs(lem[k] - l32[k]) / abs(l32[k]), abs(got[k] - l32[k]) / abs(l32[k])
        print(k, 'hip', got[k], 'emu-bf16', lem[k], 'fp32', l32[k], 'e_hip', e_hip, 'e_emu', e_emu)
    for k in got:
        e_emu, e_hip = abs(lem[k] - l32[k]) / abs(l32[k]), abs(got[k] - l32[k]) / abs(l32[k])
        assert e_hip <= (3e-2 if e_emu <= 3e-2 else 1.6 * e_emu + 5e-3), (k, e_hip, e_emu)
        assert got[k] == pytest.approx(lem[k], rel=3e-3), (k, got[k], lem[k])
    plan = next(iter(model._engine.plans.values()))
    assert torch.equal(plan.lossplan.labels.cpu(), aux32['labels'])
    named = dict(model.named_parameters())
    keys = [str(k) for k in d['grad_keys']]
    assert sorted(keys) == sorted(k for k, p in named.items() if p.requires_grad)
    bad = []
    for k in keys:
        e_hip, e_emu = rel_l2(named[k].grad.cpu(), g32[k]), rel_l2(gem[k], g32[k])
        if float(g32[k].norm()) > 0 and e_hip > 1.6 * e_emu + 5e-3:
            bad.append((k, e_hip, e_emu))
    assert not bad, bad[:10]
    got2, grad2 = step()
    assert got2 == got and torch.equal(grad2, grad)

    # train_detector from a config file: the log carries the weighted terms and their sum
    batch = dict(img=img.cuda(), img_metas=[dict(filename=f'im{i}.jpg', ori_shape=tuple(img.shape[2:]) + (3,), img_shape=tuple(img.shape[2:]) + (3,),
                                                 pad_shape=tuple(img.shape[2:]) + (3,), scale_factor=np.ones(4, np.float32), flip=False)
                                            for i in range(B)], gt_bboxes=gtb, gt_labels=gtl)

    class Loader:
        CLASSES = tuple(f'class_{i}' for i in range(80))

        def __len__(self):
            return 2

        def __iter__(self):
            return iter([batch, batch])
    cfg_file = tmp_path / 'fcos_ciou_weighted.py'
    cfg_file.write_text(
        f'model = {model_cfg!r}\n'
        'data = dict(samples_per_gpu=2, workers_per_gpu=2)\n'
        "optimizer = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.))\n"
        'optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))\n'
        "lr_config = dict(policy='step', warmup='constant', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11])\n"
        "runner = dict(type='EpochBasedRunner', max_epochs=1)\n"
        'checkpoint_config = dict(interval=1)\n'
        "log_config = dict(interval=1, hooks=[dict(type='TextLoggerHook')])\n"
        "custom_hooks = [dict(type='NumClassCheckHook')]\n"
        "log_level = 'WARNING'\nload_from = None\nresume_from = None\nworkflow = [('train', 1)]\n"
        f'work_dir = {str(tmp_path)!r}\n')
    cfg = Config.fromfile(str(cfg_file))
    fresh = build_detector(cfg.model)
    fresh.load_state_dict(sd)
    assert fresh.bbox_head.options.key() == o.key()
    runner = train_detector(fresh, [Loader()], cfg, distributed=False, validate=False)
    torch.cuda.synchronize()
    assert runner.iter == 2
    recs = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'train.log.json'))]
    recs = [r for r in recs if 'loss_cls' in r]
    assert len(recs) == 2 and all(np.isfinite(v) for r in recs for k, v in r.items() if k.startswith('loss'))
    print('logged', recs[0], 'step', got)
    for k in got:       # the first iteration is the step above (the log rounds to 4 decimals)
        assert recs[0][k] == pytest.approx(got[k], rel=1e-3, abs=2e-4), (k, recs[0][k], got[k])
    assert recs[0]['loss'] == pytest.approx(sum(got.values()), rel=1e-3, abs=5e-4)
    assert torch.isfinite(runner._det(runner.model).store.train).all()
