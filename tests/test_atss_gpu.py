"""ATSS on the GPU: dsl_atss_assign bit for bit against the reference's own assignment (tests/golden/atss_*.npz), the DSL_HEAD_ATSS
loss / detection kernels against tests/atss_ref.py (pinned to the reference by test_atss_cpu.py), one training step through
train_detector, and FPN(relu_before_extra_convs=False)."""
import json
import os

import numpy as np
import pytest
import torch

import atss_ref as AR
import aug_ref as A
from test_atss_cpu import CASES, atss_model_cfg, load_case, ref_assign
from util import levels_to_flat

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def options(c, **kw):
    from dsl_amd.params import HeadOptions
    return HeadOptions(assigner='atss', atss_topk=c['topk'], anchor_scale=c['anchor_scale'], delta_stds=c['stds'],
                       bbox_weight=c['bbox_weight'], **kw)


def assigned_plan(c, max_gt=64):
    from dsl_amd.head_loss import FcosLossPlan
    plan = FcosLossPlan(c['B'], c['sizes'], 'cuda', num_classes=c['C'], head=options(c), max_gt=max_gt)
    plan.set_targets(c['gts'], c['gls'], None, c['pads'])
    plan.assign()
    return plan


@pytest.mark.parametrize('case', CASES)
def test_assign_bit_exact_vs_reference(golden, case):
    d = golden(f'atss_{case}.npz')
    c = load_case(d)
    plan = assigned_plan(c)
    torch.cuda.synchronize()
    got = [t.cpu().clone() for t in (plan.labels, plan.assign_idx, plan.cls_weight, plan.bbox_targets, plan.npos, plan.stats, plan.pos_weight)]
    assert torch.equal(got[0], T(d['labels']).long())
    assert torch.equal(got[1], T(d['assign_idx']).int())
    assert torch.equal(got[2], T(d['cls_weight']).float())
    assert torch.equal(got[3], T(d['targets']))                    # the assigned ground-truth box, zeros elsewhere
    assert got[4].tolist() == [int(v) for v in d['npos']]
    assert float(got[5][0]) == float(d['num_total']) and float(got[5][2:].abs().max()) == 0.0
    assert float(got[5][1]) == pytest.approx(float(d['ctr_sum']), rel=1e-5)
    assert bool((got[6] == 1).all())
    # a second run (fresh plan, fresh workspace) gives the same bits; so does a rerun over the used workspace
    again = assigned_plan(c)
    plan.assign()
    torch.cuda.synchronize()
    for p in (again, plan):
        now = [t.cpu() for t in (p.labels, p.assign_idx, p.cls_weight, p.bbox_targets, p.npos, p.stats, p.pos_weight)]
        assert all(torch.equal(a, b) for a, b in zip(got, now))


def run_loss(c, cls, raw, ctr, scales):
    """Assignment + loss on flat level-major head outputs; the logits' padding columns hold NaN (they must not be read)."""
    plan = assigned_plan(c)
    C, M = c['C'], plan.M
    cl = torch.full((M, plan.LD_CLS), float('nan'))
    cl[:, :C] = cls
    rc = torch.full((M, 8), float('nan'))
    rc[:, :4], rc[:, 4] = raw, ctr
    plan.bind_outputs(cl.cuda(), rc.cuda(), scales.cuda())
    plan.loss()
    torch.cuda.synchronize()
    return plan


def check_loss(c, cls, raw, ctr, scales):
    """test_head_options_gpu.test_loss_vs_reference_golden's bars against atss_ref's float64 autograd."""
    plan = run_loss(c, cls, raw, ctr, scales)
    a = ref_assign(c)
    assert torch.equal(plan.labels.cpu(), a['labels'])
    x, r, t, s = (v.double().requires_grad_() for v in (cls, raw, ctr, scales))
    lc, lb, lt, _ = AR.loss(x, r, t, s, a, c['sizes'], c['B'], c['C'], c['anchor_scale'], c['stds'], c['bbox_weight'])
    (lc + lb + lt).backward()
    got = plan.losses.cpu()
    for i, (k, v) in enumerate((('loss_cls', lc), ('loss_bbox', lb), ('loss_centerness', lt))):
        print(k, float(got[i]), float(v.detach()))
        assert float(got[i]) == pytest.approx(float(v.detach()), rel=1e-4, abs=1e-6), k
    assert float(plan.logvec[3].cpu()) == pytest.approx(float(lc + lb + lt), rel=1e-4, abs=1e-6)
    tol = 2 ** -8
    C = c['C']
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    for mine, ref in ((mine_c[:, :C], x.grad.float()), (mine_r[:, :4], r.grad.float()), (mine_r[:, 4], t.grad.float())):
        print('max |grad err|', float((mine - ref).abs().max()), 'of', float(ref.abs().max()))
        assert torch.allclose(mine, ref, rtol=tol, atol=tol * float(ref.abs().max()) * 0.05 + 1e-9)
    assert float(mine_c[:, C:].abs().max()) == 0.0 and float(mine_r[:, 5:].abs().max()) == 0.0          # padding columns
    sgrad = s.grad.float() if s.grad is not None else torch.zeros(5)          # (no positive: the scales are not in the graph)
    assert torch.allclose(plan.g_scales.cpu()[:5], sgrad, rtol=1e-3, atol=1e-6)
    return plan, a, r.grad


@pytest.mark.parametrize('case', ['a', 'e', 'f'])
def test_loss_and_gradients_vs_float64(golden, case):
    """a: 80 classes, an active dw / dh clamp on positives (no gradient there); e: invalid anchors (weight 0); f: 18 classes (the
    partial class group), topk 3, anchor_scale 4."""
    d = golden(f'atss_{case}.npz')
    c = load_case(d)
    cls, raw, ctr = levels_to_flat(c['cls']), levels_to_flat(c['reg']), levels_to_flat(c['ctr'])[:, 0]
    plan, a, rgrad = check_loss(c, cls, raw, ctr, c['scales'])
    pos = (a['labels'] < c['C']).nonzero().view(-1)
    lvl = torch.cat([torch.full((c['B'] * h * w,), i) for i, (h, w) in enumerate(c['sizes'])])
    dwh = (raw[pos] * c['scales'][lvl[pos]][:, None])[:, 2:] * torch.tensor(c['stds'][2:])
    act = dwh.abs() > AR.MAX_RATIO
    assert bool(act.any())
    assert float(plan.g_rc.float().cpu()[pos][:, 2:4][act].abs().max()) == 0.0 and float(rgrad[pos][:, 2:][act].abs().max()) == 0.0
    if case == 'e':          # invalid anchors: no classification gradient at all
        inv = (a['cls_weight'] == 0).nonzero().view(-1)
        assert len(inv) and float(plan.g_cls.float().cpu()[inv].abs().max()) == 0.0
    again = run_loss(c, cls, raw, ctr, c['scales'])
    for u, v in ((plan.losses, again.losses), (plan.g_cls, again.g_cls), (plan.g_rc, again.g_rc), (plan.g_scales, again.g_scales)):
        assert torch.equal(u, v)


def test_loss_without_positives_has_unit_normalisers(golden):
    c = load_case(golden('atss_b.npz'))
    c['gts'], c['gls'] = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    cls, raw, ctr = levels_to_flat(c['cls']), levels_to_flat(c['reg']), levels_to_flat(c['ctr'])[:, 0]
    plan, a, _ = check_loss(c, cls, raw, ctr, c['scales'])
    assert a['npos'] == [0, 0] and plan.npos.tolist() == [0, 0]
    st = plan.stats.cpu()
    assert float(st[0]) == 2.0 and float(st[1]) == 0.0          # sum_i max(0, 1); both normalisers end at max(., 1)
    got = plan.losses.cpu()
    assert float(got[1]) == 0.0 and float(got[2]) == 0.0 and float(got[0]) > 0
    assert float(plan.g_rc.float().abs().max()) == 0.0 and bool(torch.isfinite(plan.g_cls.float()).all())


# ---- detection ------------------------------------------------------------------------------------------------------------------
def det_inputs(seed, C, n, sizes):
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(n, C, h, w, generator=g) * 2.0 - 2.0 for h, w in sizes]
    ctr = [torch.randn(n, 1, h, w, generator=g) for h, w in sizes]
    raw = [torch.randn(n, 4, h, w, generator=g) * 4.0 for h, w in sizes]
    raw[0][:, 2, ::2, ::3] = 25.0          # beyond the dw clamp
    return cls, raw, ctr


def det_plan(cls, raw, ctr, scales, C, o, n, nms_pre, iou_thr=0.6):
    from dsl_amd.sweep import DetectPlan
    sizes = [tuple(c.shape[2:]) for c in cls]
    ld = (C + 3) // 4 * 4
    flat = levels_to_flat(cls)
    cf = torch.full((flat.shape[0], ld), 30.0)
    cf[:, :C] = flat
    rc = torch.zeros(flat.shape[0], 8)
    rc[:, :4], rc[:, 4] = levels_to_flat(raw), levels_to_flat(ctr)[:, 0]
    dp = DetectPlan(n, sizes, AR.STRIDES, 'cuda', num_classes=C, nms_pre=nms_pre, ld_cls=ld, iou_thr=iou_thr, head=o)
    dp.bind(cf.cuda(), rc.cuda(), scales.cuda())
    return dp


@pytest.mark.parametrize('C,topk_scale', [(80, 8.0), (3, 4.0)])
def test_detect_vs_reference_model(C, topk_scale):
    """dsl_fcos_detect with DSL_HEAD_ATSS on fixed head outputs against atss_ref.detect, compared as
    test_head_options_gpu.test_detect_exp_decode_vs_reference compares (test_num_classes_gpu._match)."""
    from dsl_amd.params import HeadOptions
    from test_num_classes_gpu import _match
    o = HeadOptions(assigner='atss', anchor_scale=topk_scale)
    cls, raw, ctr = det_inputs(3 + C, C, 2, AR.SIZES)
    scales = torch.tensor([1.0, 0.9, 1.1, 0.8, 1.2])
    shapes = [(128, 160), (120, 150)]
    dp = det_plan(cls, raw, ctr, scales, C, o, 2, nms_pre=100)
    dp.set_meta(shapes, [1.0, 1.0], False)
    dp.run()
    torch.cuda.synchronize()
    ref = AR.detect(cls, raw, ctr, scales, shapes, nms_pre=100, iou_thr=0.6, anchor_scale=topk_scale)
    assert all(len(r[0]) >= 10 for r in ref)
    _match(dp.dets, dp.labels, dp.count, ref, 2)
    # clipped to the image shape of the second image
    k = int(dp.count[1])
    b = dp.dets[1, :k, :4].cpu()
    assert float(b[:, [0, 2]].max()) <= 150.0 and float(b[:, [1, 3]].max()) <= 120.0 and float(b.min()) >= 0.0


def test_two_view_tta_merge_vs_reference_model():
    """[view, its horizontally flipped second view at another scale] through dsl_fcos_detect_collect / _finish (aug_test's path)."""
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import AugMerge
    C, o = 5, HeadOptions(assigner='atss')
    scales = torch.tensor([1.0, 0.9, 1.1, 0.8, 1.2])
    sizes_b = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]
    views = [det_inputs(21, C, 1, AR.SIZES), det_inputs(22, C, 1, sizes_b)]
    metas = [dict(img_shape=(128, 160, 3), scale_factor=np.asarray([1.25, 1.2, 1.25, 1.2], np.float32), flip=False, flip_direction=None),
             dict(img_shape=(96, 128, 3), scale_factor=np.asarray([1.0, 0.9, 1.0, 0.9], np.float32), flip=True, flip_direction='horizontal')]
    mg = AugMerge(2, 5, 'cuda', num_classes=C, nms_pre=50, iou_thr=0.6)
    rows, plans = [], []
    for i, (v, m) in enumerate(zip(views, metas)):
        plans.append(det_plan(*v, scales, C, o, 1, nms_pre=50))
        mg.collect(i, plans[-1], m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'])
        rows.append(AR.collect(*v, scales, m['img_shape'], m['scale_factor'], m['flip_direction'] if m['flip'] else None, 50))
    dets, labels, count = mg.finish(True)
    torch.cuda.synchronize()
    k = int(count[0])
    ref_b, ref_l, _ = A.finish(torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows]), torch.cat([r[2] for r in rows]),
                               score_thr=0.05, iou_thr=0.6, max_per_img=100, cap=16384)
    assert len(ref_b) >= 10
    A.match(dets[0, :k], labels[0, :k], ref_b, ref_l)


# ---- the model ------------------------------------------------------------------------------------------------------------------
H, W = 128, 160


def make_batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    img = (torch.randn(2, 3, H, W, generator=g) * 40.0).bfloat16().float()
    gtb = [torch.tensor([[10., 12., 90., 100.], [60., 20., 150., 70.], [5., 70., 60., 120.]]), torch.tensor([[30., 30., 120., 90.]])]
    gtl = [torch.tensor([3, 17, 60]), torch.tensor([42])]
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=np.ones(4, np.float32), flip=False),
             dict(img_shape=(96, 128, 3), pad_shape=(96, 128, 3), scale_factor=np.ones(4, np.float32), flip=False)]
    return dict(img=img.cuda(), img_metas=metas, gt_bboxes=gtb, gt_labels=gtl)


class OneBatch:
    def __init__(self, batch):
        self.batch = batch

    def __len__(self):
        return 1

    def __iter__(self):
        return iter([self.batch])


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """The ATSS model after ONE iteration of train_detector (configs/atss's optimizer), with the step's log record."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config, build_detector
    work = str(tmp_path_factory.mktemp('atss'))
    model = build_detector(atss_model_cfg())
    cfg = Config(dict(
        model=atss_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001), optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001, step=[8, 11]),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=work))
    before = model.store.train.clone()
    batch = make_batch()
    runner = train_detector(model, [OneBatch(batch)], cfg, distributed=False, validate=False)
    torch.cuda.synchronize()
    recs = [json.loads(line) for line in open(os.path.join(work, 'train.log.json')) if 'loss' in line]
    return dict(model=model, batch=batch, rec=recs[-1], runner=runner, before=before)


def test_one_training_step_vs_reference_model(trained):
    """The logged losses against atss_ref evaluated on the device's own logits: rel 3e-3
    (test_head_options_gpu.test_plain_train_step_vs_reference_and_restatement's bar against its restatement)."""
    model, batch, rec = trained['model'], trained['batch'], trained['rec']
    assert trained['runner'].iter == 1
    plan = [p for p in model._engine.plans.values() if p.training][0]
    lp = plan.lossplan
    assert lp.atss is not None and plan.p6_relu is False
    sizes = [tuple(s) for s in plan.level_sizes]
    assert sizes == AR.SIZES
    pads = [m['pad_shape'][:2] for m in batch['img_metas']]
    a = AR.assign(sizes, batch['gt_bboxes'], batch['gt_labels'], pads)
    assert torch.equal(lp.labels.cpu(), a['labels']) and torch.equal(lp.assign_idx.cpu(), a['assign_idx'])
    assert torch.equal(lp.cls_weight.cpu(), a['cls_weight']) and lp.npos.tolist() == a['npos'] and min(a['npos']) > 0
    logits, rc = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu()
    scales = torch.ones(5)            # the step's forward pass ran with the initial Scale parameters
    lc, lb, lt, _ = AR.loss(logits[:, :80], rc[:, :4], rc[:, 4], scales, a, sizes, 2, 80, bbox_weight=2.0)
    for k, v in (('loss_cls', lc), ('loss_bbox', lb), ('loss_centerness', lt)):
        print(k, rec[k], float(v))
        assert rec[k] == pytest.approx(float(v), rel=3e-3), k
    assert rec['loss'] == pytest.approx(float(lc + lb + lt), rel=3e-3)
    # the optimizer moved the head, the scales and the neck; everything stayed finite
    st = model.store
    assert bool(torch.isfinite(st.train).all())
    for name in ('head.cls_w', 'head.regctr_w', 'head.scales', 'neck.fpn_convs.4.conv.weight', 'bbox_head.reg_convs.0.conv.weight'):
        off, n, _ = st.train_regions[name]
        assert not torch.equal(st.train[off:off + n].cpu(), trained['before'][off:off + n].cpu()), name


def test_simple_test_and_aug_test_run_on_the_atss_model(trained):
    model, batch = trained['model'], trained['batch']
    res = model.simple_test(batch['img'], batch['img_metas'], rescale=False)
    assert len(res) == 2 and all(len(r) == 80 for r in res)
    views = [batch['img'][:1], batch['img'][:1].flip(3)]
    metas = [[dict(batch['img_metas'][0])], [dict(batch['img_metas'][0], flip=True, flip_direction='horizontal')]]
    out = model.aug_test(views, metas, rescale=True)
    assert len(out) == 1 and len(out[0]) == 80
    got = np.concatenate(out[0])
    assert np.isfinite(got).all() and (len(got) == 0 or (got[:, :4].min() >= 0 and got[:, 2].max() <= W and got[:, 3].max() <= H))


def test_fpn_without_relu_before_extra_convs(trained):
    """P7 = fpn_convs[4](P6) on a P6 with negative entries against torch's conv2d on the bf16-rounded operands, and the data
    gradient that reaches P6 (tests/test_kernels_gpu.py's convolution bars: forward rtol / atol 1e-2, data gradient rtol 1e-2,
    atol 2e-2 of the largest reference entry)."""
    model, batch = trained['model'], trained['batch']
    model.store.grad.zero_()
    losses = model.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'])
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    plan = [p for p in model._engine.plans.values() if p.training][0]
    (h6, w6), (h7, w7) = plan.level_sizes[3], plan.level_sizes[4]
    off = plan.seg_off

    def seg(buf, i, h, w):
        return buf[off[i]:off[i] + 2 * h * w].float().cpu().view(2, h, w, 256).permute(0, 3, 1, 2)
    p6, p7 = seg(plan.bufs['feats'], 3, h6, w6), seg(plan.bufs['feats'], 4, h7, w7)
    assert int((p6 < 0).sum()) > 100
    sd = model.state_dict()
    wgt = sd['neck.fpn_convs.4.conv.weight'].bfloat16().float().cpu()
    bias = sd['neck.fpn_convs.4.conv.bias'].float().cpu()
    x = p6.clone().requires_grad_()
    ref = torch.nn.functional.conv2d(x, wgt, bias, stride=2, padding=1)
    assert torch.allclose(p7, ref.detach(), rtol=1e-2, atol=1e-2), (p7 - ref).abs().max()
    g7, g6_head = seg(plan.bufs['g_feats'], 4, h7, w7), seg(plan.bufs['g_feats'], 3, h6, w6)
    ref.backward(g7)
    want = x.grad + g6_head
    got = plan.bufs['g_p6'].float().cpu().view(2, h6, w6, 256).permute(0, 3, 1, 2)
    assert torch.allclose(got, want, rtol=1e-2, atol=2e-2 * float(want.abs().max())), (got - want).abs().max()
    neg = p6 < 0
    through = got - g6_head            # what came down from P7
    assert float(x.grad[neg].abs().max()) > 0 and int((through[neg] != 0).sum()) > 0.25 * int((x.grad[neg] != 0).sum())
