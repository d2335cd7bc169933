"""GFL on the GPU: dsl_gfl_quality / dsl_gfl_loss and the DSL_HEAD_GFL detection against tests/gfl_ref.py in float64 (pinned to the
reference's own GFLHead by test_gfl_cpu.py) on the fixtures tests/golden/gfl_*.npz, the box predictor's three convolutions at
4 (reg_max + 1) = 68 rows against a float64 convolution, one training step through train_detector, and FCOS / ATSS models beside a
GFL model in one process."""
import json
import os

import numpy as np
import pytest
import torch

import atss_ref as AR
import aug_ref as A
import gfl_ref as GR
from test_atss_gpu import H, W, OneBatch, make_batch
from test_gfl_cpu import gfl_model_cfg, load_case, loss_kw, ref_assign
from util import levels_to_flat

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def options(c):
    from dsl_amd.params import HeadOptions
    return HeadOptions(head_kind='gfl', reg_max=c['reg_max'], qfl_beta=c['beta'], dfl_weight=c['dfl_weight'], cls_weight=c['cls_weight'],
                       bbox_weight=c['bbox_weight'], box_loss=c['box_kind'], atss_topk=c['topk'], anchor_scale=c['anchor_scale'])


def run_quality(c, cls, raw, scales):
    """Assignment + quality pass on flat level-major head outputs; the logits' padding columns hold NaN (they must not be read)."""
    from dsl_amd.head_loss import FcosLossPlan
    plan = FcosLossPlan(c['B'], c['sizes'], 'cuda', num_classes=c['C'], head=options(c), max_gt=64)
    plan.set_targets(c['gts'], c['gls'], None, c['pads'])
    plan.assign()
    cl = torch.full((plan.M, plan.LD_CLS), float('nan'))
    cl[:, :c['C']] = cls
    plan.bind_outputs(cl.cuda(), raw.contiguous().cuda(), scales.cuda())
    plan.quality()
    torch.cuda.synchronize()
    return plan


def flat(c):
    return levels_to_flat(c['cls']), levels_to_flat(c['reg'])


@pytest.mark.parametrize('case', ['a', 'c', 'd', 'e'])
def test_quality_pass_vs_float64(golden, case):
    """score is an fp32 IoU of fp32 softmax expectations (rel 1e-5 + 1e-6: a handful of roundings at 2^-24 each), the weight one
    fp32 sigmoid (rel 2e-6), stats[1] their sum over at most a few hundred terms (rel 1e-5)."""
    c = load_case(golden(f'gfl_{case}.npz'))
    cls, raw = flat(c)
    plan = run_quality(c, cls, raw, c['scales'])
    a = ref_assign(c)
    assert torch.equal(plan.labels.cpu(), a['labels'])
    score, weight, wsum = GR.quality(cls.double(), raw.double(), c['scales'].double(), a, c['sizes'], c['B'], c['reg_max'], c['C'])
    got_s, got_w, st = plan.score.cpu(), plan.weight.cpu(), plan.stats.cpu()
    pos = (a['labels'] < c['C']).nonzero().view(-1)
    assert len(pos) > 0
    print('max |score err|', float((got_s.double() - score).abs().max()), 'max |w err|', float((got_w.double() - weight).abs().max()))
    assert torch.allclose(got_s.double(), score, rtol=1e-5, atol=1e-6) and torch.allclose(got_w.double(), weight, rtol=2e-6, atol=0)
    off = torch.ones(plan.M, dtype=torch.bool)
    off[pos] = False
    assert float(got_s[off].abs().max()) == 0.0 and float(got_w[off].abs().max()) == 0.0
    assert float(st[1]) == pytest.approx(float(wsum), rel=1e-5) and float(st[0]) == float(a['num_total'])
    again = run_quality(c, cls, raw, c['scales'])
    plan.quality()
    torch.cuda.synchronize()
    for p in (again, plan):
        assert torch.equal(p.score.cpu(), got_s) and torch.equal(p.weight.cpu(), got_w) and torch.equal(p.stats.cpu(), st)


def run_loss(c, cls, raw, scales, inv_world=1.0, norm_scale=None):
    plan = run_quality(c, cls, raw, scales)
    if norm_scale is not None:
        from dsl_amd import ops
        plan.norm2 = plan.stats * norm_scale
        ops.set_ptrs(plan.desc, norm=plan.norm2)
        plan.configure(inv_world=inv_world)
    plan.loss()
    torch.cuda.synchronize()
    return plan


def check_loss(c, cls, raw, scales):
    """test_atss_gpu.check_loss's bars against gfl_ref's float64 autograd: losses rel 1e-4 / abs 1e-6, bf16 gradients 2^-8."""
    plan = run_loss(c, cls, raw, scales)
    a = ref_assign(c)
    x, r, s = (v.double().requires_grad_() for v in (cls, raw, scales))
    lc, lb, ld, _ = GR.loss(x, r, s, a, c['sizes'], c['B'], **loss_kw(c))
    (lc + lb + ld).backward()
    got = plan.losses.cpu()
    for i, (k, v) in enumerate((('loss_cls', lc), ('loss_bbox', lb), ('loss_dfl', ld))):
        print(k, float(got[i]), float(v.detach()))
        assert float(got[i]) == pytest.approx(float(v.detach()), rel=1e-4, abs=1e-6), k
    assert float(got[3]) == 0.0
    assert float(plan.logvec[3].cpu()) == pytest.approx(float(lc + lb + ld), rel=1e-4, abs=1e-6) and len(plan.logvec) == 4
    tol = 2 ** -8
    C, R4 = c['C'], 4 * (c['reg_max'] + 1)
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    for mine, ref in ((mine_c[:, :C], x.grad.float()), (mine_r[:, :R4], r.grad.float())):
        print('max |grad err|', float((mine - ref).abs().max()), 'of', float(ref.abs().max()))
        assert torch.allclose(mine, ref, rtol=tol, atol=tol * float(ref.abs().max()) * 0.05 + 1e-9)
    assert float(mine_c[:, C:].abs().max()) == 0.0          # padding columns
    if plan.LD_GRC > R4:
        assert float(mine_r[:, R4:].abs().max()) == 0.0
    sgrad = s.grad.float() if s.grad is not None else torch.zeros(5)          # (no positive: the scales are not in the graph)
    assert torch.allclose(plan.g_scales.cpu()[:5], sgrad, rtol=1e-3, atol=1e-6)
    off = (a['labels'] >= C).nonzero().view(-1)
    assert float(mine_r[off].abs().max()) == 0.0
    return plan, a


@pytest.mark.parametrize('case', ['a', 'c', 'd', 'f'])
def test_loss_and_gradients_vs_float64(golden, case):
    """a: 80 classes, 68 box logits in 128 gradient columns; c: 64 logits in 64 columns; d: reg_max 3 with clamped DFL targets;
    f: beta 1.5 (powf), DFL weight 0.5, DIoU."""
    c = load_case(golden(f'gfl_{case}.npz'))
    cls, raw = flat(c)
    plan, _ = check_loss(c, cls, raw, c['scales'])
    assert (plan.LD_RC, plan.LD_GRC) == {'a': (68, 128), 'c': (64, 64), 'd': (16, 64), 'f': (68, 128)}[case]
    again = run_loss(c, cls, raw, c['scales'])
    for u, v in ((plan.losses, again.losses), (plan.g_cls, again.g_cls), (plan.g_rc, again.g_rc), (plan.g_scales, again.g_scales)):
        assert torch.equal(u, v)


def test_gradient_rows_are_rewritten_every_step(golden):
    """A location that was positive in the last step and is not in this one gets its whole row zeroed: the loss pass runs over a
    gradient buffer full of ones."""
    c = load_case(golden('gfl_a.npz'))
    cls, raw = flat(c)
    plan = run_quality(c, cls, raw, c['scales'])
    plan.g_rc.fill_(1.0)
    plan.loss()
    torch.cuda.synchronize()
    g = plan.g_rc.float().cpu()
    off = (plan.labels.cpu() >= c['C']).nonzero().view(-1)
    assert float(g[off].abs().max()) == 0.0
    # ... and a positive's row is rewritten whole: its 68 values, and zeros in the padding columns
    assert plan.LD_GRC == 128 and float(g[:, 68:].abs().max()) == 0.0
    fresh = run_loss(c, cls, raw, c['scales'])
    assert torch.equal(plan.g_rc, fresh.g_rc)


@pytest.mark.parametrize('box_kind', ['giou', 'iou'])
def test_default_loss_family_of_a_gfl_head(golden, box_kind):
    """Unit loss weights and GIoULoss / IoULoss - HeadOptions.loss_is_default() - on case c: the descriptor carries the settings all
    the same, and all three terms and their gradients are gfl_ref's (a zero-filled w_cls / w_bbox would give zero terms)."""
    c = load_case(golden('gfl_c.npz'))
    c['bbox_weight'], c['box_kind'] = 1.0, box_kind
    assert options(c).loss_is_default()
    cls, raw = flat(c)
    plan, _ = check_loss(c, cls, raw, c['scales'])
    got = plan.losses.cpu()
    assert float(got[0]) > 0.1 and float(got[1]) > 0.1 and float(got[2]) > 0.1
    assert float(plan.g_cls.float().abs().max()) > 0 and (plan.desc.w_cls, plan.desc.w_bbox) == (1.0, 1.0)


def test_image_without_positives_and_batch_without_boxes(golden):
    c = load_case(golden('gfl_b.npz'))
    cls, raw = flat(c)
    plan, a = check_loss(c, cls, raw, c['scales'])
    assert a['npos'][1] == 0 and plan.npos.tolist() == a['npos']
    assert bool(torch.isfinite(plan.losses).all()) and bool(torch.isfinite(plan.g_cls.float()).all())
    c['gts'], c['gls'] = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    plan, a = check_loss(c, cls, raw, c['scales'])
    st, got = plan.stats.cpu(), plan.losses.cpu()
    assert plan.npos.tolist() == [0, 0] and float(st[0]) == 2.0 and float(st[1]) == 0.0          # both normalisers end at max(., 1)
    assert float(got[1]) == 0.0 and float(got[2]) == 0.0 and float(got[0]) > 0 and bool(torch.isfinite(got).all())
    assert float(plan.g_rc.float().abs().max()) == 0.0 and bool(torch.isfinite(plan.g_cls.float()).all())
    assert float(plan.score.abs().max()) == 0.0 and float(plan.weight.abs().max()) == 0.0


def test_two_ranks_with_doubled_sums_reproduce_one_rank(golden):
    c = load_case(golden('gfl_d.npz'))
    cls, raw = flat(c)
    one = run_loss(c, cls, raw, c['scales'])
    two = run_loss(c, cls, raw, c['scales'], inv_world=0.5, norm_scale=2.0)
    for u, v in ((one.losses, two.losses), (one.g_cls, two.g_cls), (one.g_rc, two.g_rc), (one.g_scales, two.g_scales), (one.logvec, two.logvec)):
        assert torch.equal(u, v)


def test_wrong_descriptors_are_refused(golden):
    import ctypes as C_
    from dsl_amd import _lib as L
    c = load_case(golden('gfl_d.npz'))
    cls, raw = flat(c)
    plan = run_quality(c, cls, raw, c['scales'])
    with pytest.raises(RuntimeError, match='dsl_gfl_loss'):          # a GFL descriptor does not go through the FCOS loss
        L.check(L.lib.dsl_fcos_loss(C_.byref(plan.desc), L.stream_ptr()), 'dsl_fcos_loss')
    plan.gfl.reg_max = 17
    with pytest.raises(RuntimeError, match='reg_max'):
        plan.loss()
    plan.gfl.reg_max = c['reg_max']
    plan.desc.ld_grc = 48
    with pytest.raises(RuntimeError, match='ld_grc'):
        plan.loss()


# ---- detection ------------------------------------------------------------------------------------------------------------------
def det_inputs(seed, C, n, sizes, reg_max):
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(n, C, h, w, generator=g) * 2.0 - 2.0 for h, w in sizes]
    raw = [torch.randn(n, 4 * (reg_max + 1), h, w, generator=g) * 3.0 for h, w in sizes]
    return cls, raw


def det_plan(cls, raw, scales, C, reg_max, n, nms_pre, iou_thr=0.6):
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import DetectPlan
    sizes = [tuple(c.shape[2:]) for c in cls]
    ld = (C + 3) // 4 * 4
    fl = levels_to_flat(cls)
    cf = torch.full((fl.shape[0], ld), 30.0)
    cf[:, :C] = fl
    dp = DetectPlan(n, sizes, AR.STRIDES, 'cuda', num_classes=C, nms_pre=nms_pre, ld_cls=ld, iou_thr=iou_thr,
                    head=HeadOptions(head_kind='gfl', reg_max=reg_max))
    dp.bind(cf.cuda(), levels_to_flat(raw).contiguous().cuda(), scales.cuda())
    return dp


@pytest.mark.parametrize('C,reg_max', [(80, 16), (3, 3)])
def test_detect_vs_reference_model(C, reg_max):
    """dsl_fcos_detect with DSL_HEAD_GFL on fixed head outputs against gfl_ref.detect, compared as test_atss_gpu compares."""
    from test_num_classes_gpu import _match
    cls, raw = det_inputs(3 + C, C, 2, AR.SIZES, reg_max)
    scales = torch.tensor([1.0, 0.9, 1.1, 0.8, 1.2])
    shapes = [(128, 160), (120, 150)]
    dp = det_plan(cls, raw, scales, C, reg_max, 2, nms_pre=100)
    dp.set_meta(shapes, [1.0, 1.0], False)
    dp.run()
    torch.cuda.synchronize()
    ref = GR.detect(cls, raw, scales, shapes, reg_max, nms_pre=100, iou_thr=0.6)
    assert all(len(r[0]) >= 10 for r in ref)
    _match(dp.dets, dp.labels, dp.count, ref, 2)
    k = int(dp.count[1])
    b = dp.dets[1, :k, :4].cpu()
    assert float(b[:, [0, 2]].max()) <= 150.0 and float(b[:, [1, 3]].max()) <= 120.0 and float(b.min()) >= 0.0


def test_two_view_tta_merge_vs_reference_model():
    """[view, its horizontally flipped second view at another scale] through dsl_fcos_detect_collect / _finish (aug_test's path)."""
    from dsl_amd.sweep import AugMerge
    C, reg_max = 5, 16
    scales = torch.tensor([1.0, 0.9, 1.1, 0.8, 1.2])
    sizes_b = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]
    views = [det_inputs(21, C, 1, AR.SIZES, reg_max), det_inputs(22, C, 1, sizes_b, reg_max)]
    metas = [dict(img_shape=(128, 160, 3), scale_factor=np.asarray([1.25, 1.2, 1.25, 1.2], np.float32), flip=False, flip_direction=None),
             dict(img_shape=(96, 128, 3), scale_factor=np.asarray([1.0, 0.9, 1.0, 0.9], np.float32), flip=True, flip_direction='horizontal')]
    mg = AugMerge(2, 5, 'cuda', num_classes=C, nms_pre=50, iou_thr=0.6)
    rows, plans = [], []
    for i, (v, m) in enumerate(zip(views, metas)):
        plans.append(det_plan(*v, scales, C, reg_max, 1, nms_pre=50))
        mg.collect(i, plans[-1], m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'])
        rows.append(GR.collect(*v, scales, m['img_shape'], m['scale_factor'], m['flip_direction'] if m['flip'] else None, 50, reg_max))
    dets, labels, count = mg.finish(True)
    torch.cuda.synchronize()
    k = int(count[0])
    ref_b, ref_l, _ = A.finish(torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows]), torch.cat([r[2] for r in rows]),
                               score_thr=0.05, iou_thr=0.6, max_per_img=100, cap=16384)
    assert len(ref_b) >= 10
    A.match(dets[0, :k], labels[0, :k], ref_b, ref_l)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """An FCOS and an ATSS model's step before a GFL model exists in the process, then the GFL model after ONE iteration of
    train_detector (configs/gfl's optimizer) with the step's log record."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config, build_detector
    from test_atss_cpu import atss_model_cfg
    from util import fcos_model_cfg
    batch = make_batch()
    others = {k: build_detector(cfg).cuda() for k, cfg in (('fcos', fcos_model_cfg()), ('atss', atss_model_cfg()))}
    before = {k: one_step(m, batch) for k, m in others.items()}
    work = str(tmp_path_factory.mktemp('gfl'))
    model = build_detector(gfl_model_cfg())
    cfg = Config(dict(
        model=gfl_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001), optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001, step=[8, 11]),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=work))
    start = model.store.train.clone()
    runner = train_detector(model, [OneBatch(batch)], cfg, distributed=False, validate=False)
    torch.cuda.synchronize()
    recs = [json.loads(line) for line in open(os.path.join(work, 'train.log.json')) if 'loss' in line]
    return dict(model=model, batch=batch, rec=recs[-1], runner=runner, start=start, others=others, before=before)


def one_step(model, batch):
    """Losses and the flat gradient of one forward_train + backward."""
    model.store.grad.zero_()
    losses = model.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'])
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return {k: float(v) for k, v in losses.items()}, model.store.grad.clone()


def test_one_training_step_vs_reference_model(trained):
    """The logged losses against gfl_ref evaluated on the device's own logits: rel 3e-3 (test_atss_gpu's bar for the same check)."""
    model, batch, rec = trained['model'], trained['batch'], trained['rec']
    assert trained['runner'].iter == 1 and set(k for k in rec if k.startswith('loss')) == {'loss_cls', 'loss_bbox', 'loss_dfl', 'loss'}
    plan = [p for p in model._engine.plans.values() if p.training][0]
    lp = plan.lossplan
    assert lp.gfl is not None and lp.atss is not None and plan.p6_relu is False and plan.quality_ops is not None
    sizes = [tuple(s) for s in plan.level_sizes]
    assert sizes == AR.SIZES
    pads = [m['pad_shape'][:2] for m in batch['img_metas']]
    a = AR.assign(sizes, batch['gt_bboxes'], batch['gt_labels'], pads)
    assert torch.equal(lp.labels.cpu(), a['labels']) and lp.npos.tolist() == a['npos'] and min(a['npos']) > 0
    logits, rc = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu()
    assert tuple(rc.shape) == (plan.M, 68)
    scales = torch.ones(5)            # the step's forward pass ran with the initial Scale parameters
    lc, lb, ld, (_, _, wsum) = GR.loss(logits[:, :80].double(), rc.double(), scales.double(), a, sizes, 2)
    for k, v in (('loss_cls', lc), ('loss_bbox', lb), ('loss_dfl', ld)):
        print(k, rec[k], float(v))
        assert rec[k] == pytest.approx(float(v), rel=3e-3), k
    assert rec['loss'] == pytest.approx(float(lc + lb + ld), rel=3e-3)
    assert float(lp.stats[1].cpu()) == pytest.approx(float(wsum), rel=1e-5)
    st = model.store
    assert bool(torch.isfinite(st.train).all())
    for name in ('head.cls_w', 'head.regctr_w', 'head.regctr_b', 'head.scales', 'neck.fpn_convs.4.conv.weight', 'bbox_head.reg_convs.0.conv.weight'):
        off, n, _ = st.train_regions[name]
        assert not torch.equal(st.train[off:off + n].cpu(), trained['start'][off:off + n].cpu()), name
    assert float(st.tview('head.regctr_w')[68:].abs().max()) == 0.0 and float(st.tview('head.regctr_b')[68:].abs().max()) == 0.0


def test_box_predictor_convolutions_at_68_rows(trained):
    """Forward, weight gradient and data gradient of gfl_reg (68 of 128 stored rows) on the 128 x 160 canvas against float64
    convolutions of the bf16-rounded operands (tests/test_kernels_gpu.py's convolution bars: forward rtol / atol 1e-2; gradients
    rtol 1e-2, atol 2e-2 of the largest reference entry)."""
    from dsl_amd.engine import OpList
    model, batch = trained['model'], trained['batch']
    one_step(model, batch)
    plan = [p for p in model._engine.plans.values() if p.training][0]
    st, lp, N = model.store, plan.lossplan, 2
    sd = model.state_dict()
    wgt, bias = sd['bbox_head.gfl_reg.weight'].bfloat16().double().cpu(), sd['bbox_head.gfl_reg.bias'].double().cpu()
    act = plan.tower['reg_convs'][3]['act'].double().cpu()
    rc, g_rc = plan.bufs['regctr'].double().cpu(), lp.g_rc.double().cpu()
    assert float(g_rc[:, 68:].abs().max()) == 0.0 and float(g_rc[:, :68].abs().max()) > 0
    g_act = torch.zeros(plan.M, 256, dtype=torch.bfloat16, device='cuda')
    ol = OpList()
    ol.conv(plan._dgrad('head.regctr', lp.g_rc, g_act, N, plan.level_sizes, plan.level_sizes, cs=st.reg_pad, cd=256, k=3, stride=1, pad=1,
                        cs_real=st.reg_rows))
    ol.run()
    torch.cuda.synchronize()
    g_act = g_act.double().cpu()
    gw = st.tview('head.regctr_w', st.grad).double().cpu().permute(0, 3, 1, 2)
    gb = st.tview('head.regctr_b', st.grad).double().cpu()
    assert float(gw[68:].abs().max()) == 0.0 and float(gb[68:].abs().max()) == 0.0
    want_w, want_b, o = torch.zeros(68, 256, 3, 3, dtype=torch.float64), torch.zeros(68, dtype=torch.float64), 0
    for h, w in plan.level_sizes:
        n = N * h * w
        x = act[o:o + n].view(N, h, w, 256).permute(0, 3, 1, 2).clone().requires_grad_()
        wl = wgt.clone().requires_grad_()
        y = torch.nn.functional.conv2d(x, wl, bias, padding=1)
        got = rc[o:o + n].view(N, h, w, 68).permute(0, 3, 1, 2)
        assert torch.allclose(got, y.detach(), rtol=1e-2, atol=1e-2), (got - y).abs().max()
        gy = g_rc[o:o + n, :68].view(N, h, w, 68).permute(0, 3, 1, 2)
        y.backward(gy)
        gx = g_act[o:o + n].view(N, h, w, 256).permute(0, 3, 1, 2)
        assert torch.allclose(gx, x.grad, rtol=1e-2, atol=2e-2 * float(x.grad.abs().max())), (gx - x.grad).abs().max()
        want_w += wl.grad
        want_b += gy.sum((0, 2, 3))
        o += n
    assert torch.allclose(gw[:68], want_w, rtol=1e-2, atol=2e-2 * float(want_w.abs().max())), (gw[:68] - want_w).abs().max()
    assert torch.allclose(gb[:68], want_b, rtol=1e-2, atol=2e-2 * float(want_b.abs().max()))


def test_simple_test_aug_test_and_sweep_run_on_the_gfl_model(trained):
    from dsl_amd import sweep
    model, batch = trained['model'], trained['batch']
    # a low threshold, so that the hardly trained model's scores around the 0.01 prior give boxes (set before the first detection:
    # a plan keeps the detection descriptor it was first given)
    model.test_cfg = dict(model.test_cfg, score_thr=0.001)
    res = model.simple_test(batch['img'], batch['img_metas'], rescale=False)
    assert len(res) == 2 and all(len(r) == 80 for r in res) and all(sum(len(x) for x in r) > 0 for r in res)
    views = [batch['img'][:1], batch['img'][:1].flip(3)]
    metas = [[dict(batch['img_metas'][0])], [dict(batch['img_metas'][0], flip=True, flip_direction='horizontal')]]
    out = model.aug_test(views, metas, rescale=True)
    assert len(out) == 1 and len(out[0]) == 80
    got = np.concatenate(out[0])
    assert len(got) > 0 and np.isfinite(got).all() and got[:, :4].min() >= 0 and got[:, 2].max() <= W and got[:, 3].max() <= H
    # the pseudo-label sweep's refresh (sweep.detect_device) returns boxes inside the images
    dets, labels, count = sweep.detect_device(model, batch['img'], batch['img_metas'], rescale=False)
    torch.cuda.synchronize()
    assert int(count.min()) > 0 and bool(torch.isfinite(dets).all())
    k = int(count[1])
    assert float(dets[1, :k, 2].max()) <= 128.0 and float(dets[1, :k, 3].max()) <= 96.0 and int(labels[1, :k].max()) < 80


def test_fcos_and_atss_steps_beside_a_gfl_model(trained):
    """The FCOS and the ATSS model give, after a GFL model was built and trained in the same process, the bits they gave before
    it; the ATSS losses are atss_ref's on the device's own logits (test_atss_gpu's check and bar)."""
    batch = trained['batch']
    for k, m in trained['others'].items():
        losses, grad = one_step(m, batch)
        assert losses == trained['before'][k][0] and torch.equal(grad, trained['before'][k][1]), k
        assert set(losses) == {'loss_cls', 'loss_bbox', 'loss_centerness'}
    m = trained['others']['atss']
    plan = [p for p in m._engine.plans.values() if p.training][0]
    assert plan.lossplan.gfl is None and plan.quality_ops is None and tuple(plan.bufs['regctr'].shape) == (plan.M, 8)
    pads = [x['pad_shape'][:2] for x in batch['img_metas']]
    a = AR.assign(AR.SIZES, batch['gt_bboxes'], batch['gt_labels'], pads)
    logits, rc = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu()
    lc, lb, lt, _ = AR.loss(logits[:, :80], rc[:, :4], rc[:, 4], torch.ones(5), a, AR.SIZES, 2, 80, bbox_weight=2.0)
    got = trained['before']['atss'][0]
    for k, v in (('loss_cls', lc), ('loss_bbox', lb), ('loss_centerness', lt)):
        assert got[k] == pytest.approx(float(v), rel=3e-3), k
