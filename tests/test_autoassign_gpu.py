"""AutoAssign on the GPU: dsl_aa_assign / dsl_aa_loss through the C ABI against tests/autoassign_ref.py in float64 (pinned to the
reference's own AutoAssignHead by test_autoassign_cpu.py) on the stored inputs of tests/golden/autoassign_*.npz and on generated cases
off the fixture geometry; the DSL_HEAD_AUTOASSIGN detection; what the ABI refuses; one training step through train_detector, two
ranks, and the other heads' plans beside an AutoAssign model."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import autoassign_cases as AC
import autoassign_ref as AR
from test_autoassign_cpu import CASES, aa_model_cfg, load_case, ref_loss

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def options(c):
    from dsl_amd.params import HeadOptions
    return HeadOptions(head_kind='autoassign', bbox_weight=c['bbox_weight'], pos_loss_weight=c['pos_w'], neg_loss_weight=c['neg_w'],
                       center_loss_weight=c['center_w'])


def new_plan(c, max_gt=128):
    from dsl_amd.head_loss import FcosLossPlan
    return FcosLossPlan(c['B'], c['sizes'], 'cuda', num_classes=c['C'], head=options(c), max_gt=max_gt)


def run(c, plan=None, max_gt=128):
    """Targets, assignment and loss on the case's flat level-major head outputs; the padding columns of the logits and of the box
    predictor's rows hold NaN (they must not be read).  Everything the plan's descriptor points to is kept alive on the plan."""
    plan = plan or new_plan(c, max_gt)
    M = plan.M
    cl = torch.full((M, plan.LD_CLS), float('nan'))
    cl[:, :c['C']] = c['cls']
    rc = torch.full((M, 8), float('nan'))
    rc[:, :4] = c['raw']
    rc[:, 4] = c['obj'].reshape(-1)
    plan.prior.copy_(torch.cat([c['mean'], c['sigma']]).float())
    plan._keep = (cl.cuda(), rc.cuda(), c['scales'].float().cuda())
    plan.bind_outputs(*plan._keep)
    plan.set_targets(c['gts'], c['gls'])
    plan.assign()
    plan.loss()
    torch.cuda.synchronize()
    return plan


def outputs(plan):
    return [t.detach().cpu().clone() for t in (plan.stats, plan.losses, plan.logvec, plan.g_cls, plan.g_rc, plan.g_scales, plan.g_prior, plan.iou)]


def check(plan, c, ref):
    """tests/test_atss_gpu.py::check_loss's bars: losses rel 1e-4 / abs 1e-6, head-output gradients 2^-8 relative to the bf16 storage.
    d mean / d sigma and d scale are fp32: the fixtures' 1e-4 of the tensor's largest magnitude (test_autoassign_cpu.py shows that
    fp32 arithmetic itself holds it).  Each figure is printed before it is asserted."""
    out, gc, gr, go, gs, gm, gsg = ref
    Cn = c['C']
    st, got, lv = plan.stats.cpu(), plan.losses.cpu(), plan.logvec.cpu()
    print('stats', st[:2].tolist(), out['stats'])
    assert float(st[0]) == out['stats'][0] and float(st[1]) == pytest.approx(out['stats'][1], rel=1e-5, abs=1e-6)
    assert st[2:].tolist() == [0.0] * 6
    want = [float(out[k].detach()) for k in ('loss_pos', 'loss_neg', 'loss_center')]
    for i, k in enumerate(('loss_pos', 'loss_neg', 'loss_center')):
        print(k, float(got[i]), want[i])
        assert float(got[i]) == pytest.approx(want[i], rel=1e-4, abs=1e-6), k
    assert float(got[3]) == 0.0
    assert lv.shape == (4,) and lv[:3].tolist() == got[:3].tolist() and float(lv[3]) == pytest.approx(sum(want), rel=1e-4, abs=1e-6)
    n = c['B']
    for i in range(n):
        rows = T(AR.image_rows(c['sizes'], n, i))
        err = float((plan.iou.cpu()[rows] - out['iou'][i].float()).abs().max())
        print('image', i, 'max |iou err|', err)
        assert err <= 1e-5
    tol = 2 ** -8
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    for name, mine, ref_t in (('cls', mine_c[:, :Cn], gc.float()), ('raw', mine_r[:, :4], gr.float()), ('obj', mine_r[:, 4:5], go.float().reshape(-1, 1))):
        print(name, 'max |grad err|', float((mine - ref_t).abs().max()), 'of', float(ref_t.abs().max()))
        assert torch.allclose(mine, ref_t, rtol=tol, atol=tol * float(ref_t.abs().max()) * 0.05 + 1e-9), name
    assert float(mine_c[:, Cn:].abs().max()) == 0.0 and float(mine_r[:, 5:].abs().max()) == 0.0          # padding columns
    assert bool(torch.isfinite(mine_c).all()) and bool(torch.isfinite(mine_r).all())
    gp = plan.g_prior.cpu().double()
    for name, mine, ref_t in (('mean', gp[:Cn], gm), ('sigma', gp[Cn:], gsg), ('scales', plan.g_scales.cpu().double()[:5], gs)):
        err, top = float((mine - ref_t).abs().max()), float(ref_t.abs().max())
        print('d', name, 'max err', err, 'of', top)
        assert err <= 1e-4 * max(top, 1e-30), name


# ---- 1. every fixture: stored inputs, float64 model --------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_fixture_vs_float64(case):
    """a: 80 classes (two classes per lane), a moved prior; b: an image without boxes; c: no box in the batch; d: shared points of one
    class, a box that holds no point (the -100 clamp), a box over the whole canvas; e: 18 classes, other weights."""
    c = load_case(case)
    plan = run(c)
    check(plan, c, ref_loss(case))
    if case == 'c':
        assert plan.losses.cpu().tolist()[0] == 0.0 and plan.losses.cpu().tolist()[2] == 0.0 and plan.stats[:2].tolist() == [0.0, 0.0]
        assert not bool(plan.g_prior.any()) and not bool(plan.g_rc[:, :4].any()) and not bool(plan.g_scales.any())
    # bit-identical on a second run: a fresh plan, and a rerun over the used workspace
    first = outputs(plan)
    again = run(c)
    run(c, plan)
    for p in (again, plan):
        assert all(torch.equal(u, v) for u, v in zip(first, outputs(p)))


def test_grad_scale_scales_the_gradients_only():
    c = load_case('e')
    one = run(c)
    plan = new_plan(c)
    plan.configure(grad_scale=0.25)
    run(c, plan)
    assert torch.equal(plan.losses, one.losses) and torch.equal(plan.logvec, one.logvec) and torch.equal(plan.stats, one.stats)
    for u, v in ((plan.g_cls, one.g_cls), (plan.g_rc, one.g_rc), (plan.g_scales, one.g_scales), (plan.g_prior, one.g_prior)):
        assert torch.equal(u.float(), v.float() * 0.25) and bool(v.any())          # (a power of two: exact)


def test_the_normalisers_are_the_exchanged_sums():
    """norm holds the sum over ranks of stats[0:2], inv_world their mean's factor: twice this rank's sums at inv_world 0.5 give this
    rank's losses and gradients; other sums give the model's losses under them."""
    c = load_case('d')
    one = run(c)
    plan = new_plan(c)
    plan.configure(inv_world=0.5)
    norm = torch.tensor([20.0, 300.0, 0, 0, 0, 0, 0, 0], device='cuda')
    plan.desc.norm = norm.data_ptr()
    run(c, plan)
    own = one.stats.cpu().tolist()
    want = AC.compute(c, world=(20.0, 300.0, 0.5))
    got = plan.losses.cpu().tolist()
    print(got, [float(want[0][k].detach()) for k in ('loss_pos', 'loss_neg', 'loss_center')], own)
    assert got[0] == pytest.approx(float(want[0]['loss_pos'].detach()), rel=1e-4) and got[1] == pytest.approx(float(want[0]['loss_neg'].detach()), rel=1e-4)
    assert got[2] == one.losses.cpu().tolist()[2]                       # the centre loss is not reduced between ranks
    assert got[0] == pytest.approx(one.losses.cpu().tolist()[0] * max(own[0], 1.0) / 10.0, rel=1e-5)


# ---- 2. generated cases off the fixture geometry -----------------------------------------------------------------------------------
def test_four_images_with_an_empty_one_and_a_level_of_twenty_workgroups():
    c = AC.case('four_images')
    assert c['n'] * c['sizes'][0][0] * c['sizes'][0][1] == 20 * 256 and len(c['gts'][2]) == 0
    total = sum(len(b) for b in c['gts'])
    plan = run(c, max_gt=total)          # max_gt boxes in the batch: the capacity is the only cap
    check(plan, c, AC.ref('four_images'))
    # the empty image: no positive term reaches it (its box gradients are zero), its negative weights are 1
    rows = T(AR.image_rows(c['sizes'], c['n'], 2))
    assert not bool(plan.g_rc.cpu()[rows][:, :4].any()) and not bool(plan.iou.cpu()[rows].any())


def test_seventy_boxes_in_one_image_and_a_reused_plan_with_fewer():
    c = AC.case('many_boxes')
    assert len(c['gts'][0]) == 70
    plan = run(c)
    check(plan, c, AC.ref('many_boxes'))
    # the next step of the same plan has fewer boxes: nothing of the step before survives
    f = AC.case('fewer')
    run(f, plan)
    check(plan, f, AC.ref('fewer'))
    assert float(plan.stats[0]) == 8.0          # 5 + 3 boxes


@pytest.mark.parametrize('name,C', [('many_boxes_80', 80), ('four_images_18', 18)])
def test_class_counts_off_the_fixtures(name, C):
    """80 classes with 70 boxes in an image: the lane's second class (c + 64) together with a second chunk of boxes; 18 classes (no
    multiple of 4) on the larger canvas with an empty image."""
    c = AC.case(name)
    assert c['C'] == C
    plan = run(c, max_gt=128)
    check(plan, c, AC.ref(name))
    if C == 80:
        assert len(c['gts'][0]) == 70 and bool((c['gls'][0] >= 64).any()) and bool(plan.g_cls[:, 64:80].any())


def test_one_class():
    c = AC.case('one_class')
    plan = run(c)
    check(plan, c, AC.ref('one_class'))
    assert plan.LD_CLS == 4 and float(plan.g_cls.float().abs().max()) > 0


# ---- 3. detection ------------------------------------------------------------------------------------------------------------------
def det_plan(c, n=None, views=None, **kw):
    from dsl_amd.sweep import DetectPlan
    n = n or c['B']
    Cn = c['C']
    cls, raw, obj = c['cls'], c['raw'], c['obj']
    if views is not None:
        cls, raw, obj = views
    cf = torch.full((cls.shape[0], (Cn + 3) // 4 * 4), float('nan'))
    cf[:, :Cn] = cls
    rc = torch.full((cls.shape[0], 8), float('nan'))
    rc[:, :4] = raw
    rc[:, 4] = obj.reshape(-1)
    d = c['d']
    dp = DetectPlan(n, c['sizes'], AR.STRIDES, 'cuda', num_classes=Cn, nms_pre=int(d['nms_pre']), ld_cls=cf.shape[1], head=options(c),
                    score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']), **kw)
    dp._keep = (cf.cuda(), rc.cuda(), c['scales'].float().cuda())
    dp.bind(*dp._keep)
    return dp


@pytest.mark.parametrize('rescale', [False, True])
def test_detect_vs_fixture_and_float64_decode(rescale):
    """dsl_fcos_detect with DSL_HEAD_AUTOASSIGN on fixture d's head outputs against autoassign_ref.detect (the point-origin decode in
    float64 + the project's CPU NMS model) and, with rescale, against the reference's own get_bboxes; compared as
    tests/test_atss_gpu.py::test_detect_vs_reference_model compares (test_num_classes_gpu._match)."""
    from dsl_amd import _lib as L
    from test_num_classes_gpu import _match
    c = load_case('d')
    d = c['d']
    dp = det_plan(c)
    assert dp.desc.head_flags == L.HEAD_AUTOASSIGN
    shapes, sfs = [tuple(int(v) for v in s) for s in d['img_shapes']], [float(s[0]) for s in d['scale_factors']]
    dp.set_meta(shapes, sfs, rescale)
    dp.run()
    torch.cuda.synchronize()
    cls, raw, obj = (AR.unflat(c[k].double(), c['sizes'], c['B']) for k in ('cls', 'raw', 'obj'))
    ref = AR.detect(cls, raw, obj, c['scales'].double(), shapes, list(d['scale_factors']) if rescale else None, nms_pre=int(d['nms_pre']),
                    score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']))
    ref = [(b.float(), l) for b, l in ref]
    assert all(len(r[0]) >= 10 for r in ref)
    _match(dp.dets, dp.labels, dp.count, ref, 2)
    if rescale:
        _match(dp.dets, dp.labels, dp.count, [(T(d[f'det{i}_boxes']), T(d[f'det{i}_labels'])) for i in range(2)], 2)
    # the half-stride offset would move every box by 4 .. 64 pixels: FCOS's flag-less decode does not match
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import DetectPlan
    fc = DetectPlan(2, c['sizes'], AR.STRIDES, 'cuda', num_classes=c['C'], nms_pre=int(d['nms_pre']), ld_cls=dp._keep[0].shape[1], head=HeadOptions(),
                    score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']))
    fc.bind(*dp._keep)
    fc.set_meta(shapes, sfs, rescale)
    fc.run()
    torch.cuda.synchronize()
    k = min(int(dp.count[0]), int(fc.count[0]))
    assert k > 0 and float((dp.dets[0, :k, :4] - fc.dets[0, :k, :4]).abs().max()) >= 1.0


def test_two_views_one_flipped_merge_vs_float64():
    """dsl_fcos_detect_collect / _finish with DSL_HEAD_AUTOASSIGN: fixture d's two images stand for two views of one image, the second
    one mirrored horizontally at another scale factor.  Against autoassign_ref.collect per view (point-origin decode, flip mapped
    back, division by the view's scale factor) and the project's CPU NMS model over the pooled candidates, compared as
    tests/test_aug_test_gpu.py compares (aug_ref.match): a half-stride offset or a wrong map-back moves boxes by pixels."""
    import aug_ref as A
    from dsl_amd.sweep import AugMerge
    c = load_case('d')
    d = c['d']
    shape, sfs, flips = (128, 160, 3), [np.ones(4, np.float32), np.full(4, 1.25, np.float32)], [None, 'horizontal']
    kw = dict(score_thr=float(d['score_thr']), iou_thr=float(d['iou_thr']), max_per_img=int(d['max_per_img']))
    mg = AugMerge(2, 5, 'cuda', num_classes=c['C'], nms_pre=int(d['nms_pre']), **kw)
    parts, keep = [], []
    for v in range(2):
        rows = T(AR.image_rows(c['sizes'], 2, v))
        view = tuple(c[k][rows] for k in ('cls', 'raw', 'obj'))
        dp = det_plan(c, n=1, views=view)
        keep.append(dp)
        mg.collect(v, dp, shape, sfs[v], flip=flips[v] is not None, flip_direction=flips[v])
        per_level = [AR.unflat(t.double(), c['sizes'], 1) for t in view]
        parts.append(AR.collect(*per_level, c['scales'].double(), shape, sfs[v], int(d['nms_pre']), flip_direction=flips[v]))
    dets, labels, count = mg.finish(True)
    torch.cuda.synchronize()
    k = int(count[0])
    ref_b, ref_l, _ = A.finish(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), cap=16384, **kw)
    assert k >= 20 and len(ref_b) == k
    A.match(dets[0, :k], labels[0, :k], ref_b.float(), ref_l)
    # the mirrored view contributes: some kept box comes from it (it is none of the plain view's candidates)
    plain = parts[0][0].float()
    assert bool(((dets[0, :k, None, :4].cpu() - plain[None]).abs().amax(-1).amin(1) > 1.0).any())


def test_host_labels_outside_the_prior_are_refused():
    c = dict(load_case('e'))
    plan = new_plan(c)
    bad = [c['gls'][0].clone(), c['gls'][1]]
    bad[0][0] = c['C']
    with pytest.raises(ValueError, match='gt_labels in 0..17'):
        plan.set_targets(c['gts'], bad)
    check(run(c, plan), c, ref_loss('e'))          # the plan is unharmed


def test_abi_refusals():
    from dsl_amd import _lib as L
    c = load_case('d')
    plan = run(c)
    d, f = plan.desc, plan.aa
    assert C.addressof(d) == C.addressof(f) and d.head_flags == L.HEAD_AUTOASSIGN | L.HEAD_LOSS_EXT == 1040

    def refused(fn, match):
        rc = getattr(L.lib, fn)(C.byref(d), L.stream_ptr())
        msg = L.lib.dsl_last_error().decode()
        assert rc != 0 and match in msg, (fn, rc, msg)

    keep = (d.head_flags, d.ig_boxes, d.ig_off, f.max_gt, f.w_pos, d.workspace_bytes, d.soft_weight, d.loss_weight, d.box_kind, f.mean, f.iou,
            d.num_classes, d.ld_rc, d.w_bbox, f.g_sigma)
    d.ig_boxes, d.ig_off = plan.ig_boxes.data_ptr(), plan.ig_off.data_ptr()
    for fn in ('dsl_aa_assign', 'dsl_aa_loss', 'dsl_head_assign', 'dsl_head_loss'):
        refused(fn, 'ig_boxes')
    d.ig_boxes, d.ig_off = keep[1], keep[2]
    for extra in (L.HEAD_ATSS, L.HEAD_GFL, L.HEAD_PAA, L.HEAD_LD, L.HEAD_FOVEA, L.HEAD_EXP_DECODE, L.HEAD_INSIDE_BOX):
        d.head_flags = keep[0] | extra
        refused('dsl_aa_assign', 'head_flags')
        refused('dsl_aa_loss', 'head_flags')
    d.head_flags = L.HEAD_AUTOASSIGN          # without the loss family
    refused('dsl_aa_loss', 'head_flags')
    d.head_flags = keep[0]
    refused('dsl_fcos_assign', 'DSL_HEAD_AUTOASSIGN')
    refused('dsl_fcos_loss', 'DSL_HEAD_AUTOASSIGN')
    for bad in (0, -1, (1 << 20) + 1):
        f.max_gt = bad
        refused('dsl_aa_assign', 'max_gt')
    f.max_gt = keep[3]
    for bad in (-0.5, float('inf'), float('nan')):
        f.w_pos = bad
        refused('dsl_aa_loss', 'w_pos')
    f.w_pos = keep[4]
    d.workspace_bytes = keep[5] - 1
    refused('dsl_aa_assign', 'workspace')
    refused('dsl_aa_loss', 'workspace')
    d.workspace_bytes = keep[5]
    d.soft_weight = 0.5
    refused('dsl_aa_loss', 'soft_weight')
    d.soft_weight = keep[6]
    d.loss_weight = 0.5
    refused('dsl_aa_loss', 'loss_weight')
    d.loss_weight = keep[7]
    d.box_kind = L.BOX_DIOU
    refused('dsl_aa_loss', 'box_kind')
    d.box_kind = keep[8]
    f.mean = None
    refused('dsl_aa_assign', 'mean')
    f.mean = keep[9]
    f.iou = None
    refused('dsl_aa_loss', 'iou')
    f.iou = keep[10]
    f.g_sigma = None
    refused('dsl_aa_loss', 'null pointer')
    f.g_sigma = keep[14]
    d.num_classes = 129
    refused('dsl_aa_loss', 'num_classes')
    d.num_classes = keep[11]
    d.ld_rc = 4
    refused('dsl_aa_loss', 'ld_rc')
    d.ld_rc = keep[12]
    d.w_bbox = -1.0
    refused('dsl_aa_loss', 'w_bbox')
    d.w_bbox = keep[13]
    # detection: the flag goes with no other, and with the objectness on the regression tower
    dp = det_plan(c)
    dp.set_meta([(128, 160), (100, 130)], [1.0, 1.25], False)
    dp.desc.head_flags = L.HEAD_AUTOASSIGN | L.HEAD_EXP_DECODE
    rc = L.lib.dsl_fcos_detect(C.byref(dp.desc), L.stream_ptr())
    assert rc != 0 and 'DSL_HEAD_AUTOASSIGN goes with no other flag' in L.lib.dsl_last_error().decode()
    # restored: the descriptor runs again and gives the bits of before
    before = outputs(plan)
    plan.assign()
    plan.loss()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(before, outputs(plan)))


# ---- 4. the model ------------------------------------------------------------------------------------------------------------------
def _cfg(model_cfg, work):
    from dsl_amd.registry import Config
    return Config(dict(
        model=model_cfg, data=dict(samples_per_gpu=2, workers_per_gpu=2),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001, paramwise_cfg=dict(norm_decay_mult=0.)),
        optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=1000, warmup_ratio=0.001, step=[8, 11]),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=work))


def _moved_prior(model):
    """A prior off its initial (0, 1), so that its gradients are not the symmetric special case."""
    g = torch.Generator().manual_seed(5)
    sd = model.state_dict()
    model.load_state_dict(dict(sd, **{'bbox_head.center_prior.mean': 0.3 * torch.randn(80, 2, generator=g),
                                      'bbox_head.center_prior.sigma': 1.0 + 0.5 * torch.rand(80, 2, generator=g)}))
    return model


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """The AutoAssign model after ONE iteration of train_detector (configs/autoassign's optimizer), with the step's log record."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import build_detector
    from test_atss_gpu import OneBatch, make_batch
    work = str(tmp_path_factory.mktemp('autoassign'))
    torch.manual_seed(3)
    model = _moved_prior(build_detector(aa_model_cfg()))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batch = make_batch()
    runner = train_detector(model, [OneBatch(batch)], _cfg(aa_model_cfg(), work), distributed=False, validate=False)
    torch.cuda.synchronize()
    recs = [json.loads(line) for line in open(os.path.join(work, 'train.log.json')) if 'loss' in line]
    return dict(model=model, batch=batch, rec=recs[-1], runner=runner, before=before)


def test_one_training_step(trained):
    """The logged losses are the loss kernel's, and autoassign_ref's on the device's own head outputs (rel 3e-3,
    test_atss_gpu.test_one_training_step_vs_reference_model's bar); every trainable parameter moved, the prior's among them."""
    model, batch, rec = trained['model'], trained['batch'], trained['rec']
    assert trained['runner'].iter == 1 and set(k for k in rec if k.startswith('loss')) == {'loss_pos', 'loss_neg', 'loss_center', 'loss'}
    plan = [p for p in model._engine.plans.values() if p.training][0]
    lp = plan.lossplan
    assert lp.aa is not None and lp.atss is None and lp.kind.name == 'autoassign'
    st = model.store
    assert lp.aa.mean == st.prior_ptrs()[0] and lp.aa.g_sigma == st.prior_ptrs(st.grad)[1]
    sizes = [tuple(s) for s in plan.level_sizes]
    own = lp.losses.cpu().tolist()
    logits, rc = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu()
    assert rc.shape[1] == 8 and st.reg_rows == 5
    b4 = trained['before']
    out = AR.loss(logits[:, :80].double(), rc[:, :4].double(), rc[:, 4:5].double(), torch.stack([b4[f'bbox_head.scales.{i}.scale'] for i in range(5)]).cpu().double(),
                  b4['bbox_head.center_prior.mean'].cpu().double(), b4['bbox_head.center_prior.sigma'].cpu().double(),
                  batch['gt_bboxes'], batch['gt_labels'], sizes, 80)
    for i, k in enumerate(('loss_pos', 'loss_neg', 'loss_center')):
        print(k, rec[k], own[i], float(out[k]))
        assert rec[k] == pytest.approx(own[i], rel=1e-4, abs=1e-4), k          # (the text log keeps five decimals)
        assert own[i] == pytest.approx(float(out[k]), rel=3e-3), k
    assert rec['loss'] == pytest.approx(sum(own[:3]), rel=1e-4, abs=1e-4)
    assert lp.stats[:2].cpu().tolist() == pytest.approx(list(out['stats']), rel=1e-5)
    assert bool(torch.isfinite(st.train).all())
    grads = st.named_views(st.grad)
    assert 'bbox_head.center_prior.mean' in grads and bool(grads['bbox_head.center_prior.sigma'].any())
    after = model.state_dict()
    same = [k for k in grads if torch.equal(after[k].cpu(), b4[k].cpu())]
    # The first warm-up iteration's lr is 1e-5: a Scale of exactly 1.0 moves only where its gradient exceeds half an ulp / lr = 6e-3,
    # which the coarse levels' few locations do not reach.  Everything else moved - the prior too: a class without a box in the
    # batch has no gradient, its rows still decay
    assert all(k.startswith('bbox_head.scales.') for k in same) and len(same) < 5, same
    assert all(bool(grads[f'bbox_head.scales.{i}.scale'].ne(0)) for i in range(3))


def test_ema_carries_the_prior(trained):
    """The runner's EMA is one lerp over the flat trainable buffer (dsl_ema_lerp over n_train): the prior's region is inside it."""
    from dsl_amd import _lib as L
    from dsl_amd.params import ParamStore
    st = trained['model'].store
    ema = ParamStore(80, 'cuda', head=st.head)
    assert ema.train_regions == st.train_regions and not bool(ema.train.any())
    L.check(L.lib.dsl_ema_lerp(L.ptr(ema.train), L.ptr(st.train), st.n_train, 0.75, L.stream_ptr()), 'dsl_ema_lerp')
    torch.cuda.synchronize()
    v, w = ema.named_views(), st.named_views()
    for k in ('bbox_head.center_prior.mean', 'bbox_head.center_prior.sigma'):
        assert v[k].shape == (80, 2) and bool(w[k].any()) and torch.allclose(v[k], 0.25 * w[k], rtol=1e-6, atol=0)


def test_state_dict_round_trip_simple_test_and_aug_test(trained):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    model, batch = trained['model'], trained['batch']
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert 'bbox_head.center_prior.mean' in sd and 'bbox_head.center_prior.sigma' in sd and 'bbox_head.scales.4.scale' in sd
    other = build_detector(aa_model_cfg()).cuda()
    other.load_state_dict(sd)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in other.state_dict().items())
    res = model.simple_test(batch['img'], batch['img_metas'], rescale=False)
    res2 = other.simple_test(batch['img'], batch['img_metas'], rescale=False)
    assert len(res) == 2 and all(len(r) == 80 and all(x.shape[1] == 5 and x.dtype == np.float32 for x in r) for r in res)
    assert all(np.array_equal(x, y) for r, r2 in zip(res, res2) for x, y in zip(r, r2))
    got = np.concatenate(res[0])
    assert np.isfinite(got).all() and len(got) > 0
    # aug_test with one flip: the merged detections contain the plain view's candidates (get_bboxes has with_nms: no refusal)
    views = [batch['img'][:1], batch['img'][:1].flip(3)]
    metas = [[dict(batch['img_metas'][0])], [dict(batch['img_metas'][0], flip=True, flip_direction='horizontal')]]
    aug = model.aug_test(views, metas, rescale=True)
    assert len(aug) == 1 and len(aug[0]) == 80
    merged = np.concatenate(aug[0])
    assert np.isfinite(merged).all() and len(merged) > 0 and merged[:, 4].max() == pytest.approx(got[:, 4].max(), rel=0.2)


def _half(rank):
    from test_atss_gpu import make_batch
    b = make_batch()
    if rank == 1:          # the second rank sees the images in the other order with one box fewer: other normalisers than rank 0's
        b = dict(img=b['img'].flip(0).contiguous(), img_metas=b['img_metas'][::-1], gt_bboxes=[b['gt_bboxes'][1], b['gt_bboxes'][0][:2]],
                 gt_labels=[b['gt_labels'][1], b['gt_labels'][0][:2]])
    return b


def _build_cuda():
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    torch.manual_seed(3)
    return _moved_prior(build_detector(aa_model_cfg())).cuda()


def _rank_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from dsl_amd.optim import FlatSGD
        from dsl_amd.parallel import HipDistributedDataParallel
        model = _build_cuda()
        ddp = HipDistributedDataParallel(model)
        # lr 0.2: the first step moves the prior far enough for a stale one to show in the second step's normaliser (checked below)
        opt = FlatSGD(model, lr=0.2, momentum=0.9, weight_decay=1e-4)
        batch = _half(rank)
        sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if 'center_prior' in k}
        out = ddp.train_step(batch, opt)
        plan = [p for p in model._engine.plans.values() if p.training][0]
        own_dev = plan.lossplan.losses.clone()          # (a device copy in stream order: no host synchronisation between the steps)
        out['loss'].backward()
        opt.step()
        # the second step follows at once - no synchronisation: its assignment must itself wait for the first step's late update of
        # the head + FPN bucket, which holds the prior
        out2 = ddp.train_step(batch, opt)
        out2['loss'].backward()
        model.store.wait_pending()
        torch.cuda.synchronize()
        own = own_dev.cpu().tolist()[:3]
        lp = plan.lossplan
        stats = None
        sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if 'center_prior' in k or 'scales' in k}
        logits, rc = plan.bufs['cls_logits'].cpu().double(), plan.bufs['regctr'].cpu().double()
        sizes = [tuple(s) for s in plan.level_sizes]

        def serial(mean, sigma, world=None):
            return AR.loss(logits[:, :80], rc[:, :4], rc[:, 4:5], torch.stack([sd[f'bbox_head.scales.{i}.scale'] for i in range(5)]), mean, sigma,
                           batch['gt_bboxes'], batch['gt_labels'], sizes, 80, world=world)
        mine = serial(sd['bbox_head.center_prior.mean'], sd['bbox_head.center_prior.sigma'])['stats']
        stale = serial(sd0['bbox_head.center_prior.mean'].double(), sd0['bbox_head.center_prior.sigma'].double())['stats']
        both = [None] * world
        dist.all_gather_object(both, mine)
        tot = [sum(b[0] for b in both), sum(b[1] for b in both)]
        want = serial(sd['bbox_head.center_prior.mean'], sd['bbox_head.center_prior.sigma'], world=(tot[0], tot[1], 1.0 / world))
        step2 = dict(stats=lp.stats.cpu().tolist()[:2], tot=tot, losses=lp.losses.cpu().tolist()[:3],
                     want=[float(want[k]) for k in ('loss_pos', 'loss_neg', 'loss_center')], own_sum=mine[1], stale_sum=stale[1])
        opt.step()
        model.store.wait_pending()
        torch.cuda.synchronize()
        w = model.store.train.detach().cpu()
        lst = [torch.zeros_like(w) for _ in range(world)]
        dist.all_gather(lst, w)
        same = all(torch.equal(t, lst[0]) for t in lst) and bool(torch.isfinite(w).all())
        dist.destroy_process_group()
        stats = step2
        q.put((rank, 'ok', same, own, stats))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), False, None, None))


def test_two_ranks_end_with_identical_weights_and_exchange_the_two_normalisers():
    """World size 2 on one GPU (gloo, as tests/test_ddp_gpu.py arranges it), two steps back to back: stats[0:2] hold the sum over both ranks (box count and
    sum c), the positive and negative losses are the single-process sums over the mean normalisers, the centre loss is the rank's
    own, and after the optimizer step both ranks hold the same weights."""
    import torch.multiprocessing as mp
    from test_ddp_gpu import _free_port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=150) for _ in procs)
    finally:
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
    assert all(r[1] == 'ok' for r in res), [r[1] for r in res]
    assert all(r[2] for r in res), 'ranks hold different weights'
    single, stats = [], []
    for rank in range(2):
        model = _build_cuda()
        out = model.train_step(_half(rank), None)
        torch.cuda.synchronize()
        lp = [p for p in model._engine.plans.values() if p.training][0].lossplan
        single.append([float(out['log_vars'][k]) for k in ('loss_pos', 'loss_neg', 'loss_center')])
        stats.append(lp.stats.cpu().tolist()[:2])
    tot = [stats[0][0] + stats[1][0], stats[0][1] + stats[1][1]]
    assert stats[0][0] != stats[1][0]                                   # the halves do differ
    for rank in range(2):
        # step 1: the logged losses are the single-process sums over the mean normalisers; the centre loss is the rank's own
        print(rank, res[rank][3], single[rank], tot)
        want = [single[rank][0] * max(stats[rank][0], 1.0) / max(tot[0] / 2, 1.0), single[rank][1] * max(stats[rank][1], 1.0) / max(tot[1] / 2, 1.0),
                single[rank][2]]
        assert res[rank][3] == pytest.approx(want, rel=1e-4)
        # step 2, queued right behind step 1's optimizer step: both normalisers and the three losses are the serial computation's
        # on the UPDATED prior and the step's own head outputs - and a prior of one step earlier would have shown
        s2 = res[rank][4]
        print(rank, 'step 2', s2)
        assert abs(s2['stale_sum'] - s2['own_sum']) > 1e-4 * s2['own_sum'], 'the first step did not move the prior enough to tell'
        assert s2['stats'] == pytest.approx(s2['tot'], rel=1e-5)
        assert s2['losses'] == pytest.approx(s2['want'], rel=1e-3)


# ---- 5. the new kind leaks into nothing ----------------------------------------------------------------------------------------------
def _signature(cfg_fn):
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tools')) if p not in sys.path]
    import plan_signature as PS
    model, opt = PS.build_model(getattr(PS, cfg_fn))
    eng = model._get_engine()
    plan = eng.plan(model.store, 2, 64, 96, training=True)
    torch.cuda.synchronize()
    lines = []
    PS.signature(plan, {'engine': eng, 'plan': plan, 'store': model.store, 'opt': opt, 'pixtabs': PS.ops._pixtabs, 'model': model}, lines.append)
    return '\n'.join(lines)


@pytest.mark.parametrize('cfg_fn', ['resnet_cfg', 'atss_cfg'])
def test_plan_signature_beside_an_autoassign_model(cfg_fn):
    before = _signature(cfg_fn)
    model = _build_cuda()
    plan = model._get_engine().plan(model.store, 2, 64, 96, training=True)
    assert plan.lossplan.kind.name == 'autoassign'
    torch.cuda.synchronize()
    after = _signature(cfg_fn)
    assert len(before.splitlines()) > 100 and before == after
