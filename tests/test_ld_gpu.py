"""LD on the GPU: dsl_ld_loss against tests/ld_ref.py in float64 (pinned to the reference's own LDHead by test_ld_cpu.py) on the
fixtures tests/golden/ld_*.npz, its relation to dsl_gfl_loss (w_ld = 0, teacher == student), its refusals, one training step of the
distillation detector through train_detector, GFL / FCOS / ATSS models beside it in one process, and inference."""
import ctypes as C_
import json
import os

import pytest
import torch

import atss_ref as AR
import gfl_ref as GR
import ld_ref as LR
from test_atss_gpu import OneBatch, make_batch
from test_gfl_cpu import gfl_model_cfg, loss_kw, ref_assign
from test_gfl_gpu import one_step
from test_ld_cpu import ld_kw, ld_model_cfg, load_case
from util import levels_to_flat

pytestmark = pytest.mark.gpu


def options(c, ld=True):
    from dsl_amd.params import HeadOptions
    return HeadOptions(head_kind='gfl', reg_max=c['reg_max'], qfl_beta=c['beta'], dfl_weight=c['dfl_weight'], cls_weight=c['cls_weight'],
                       bbox_weight=c['bbox_weight'], box_loss=c['box_kind'], atss_topk=c['topk'], anchor_scale=c['anchor_scale'],
                       ld_weight=c['ld_weight'] if ld else None, ld_T=c['T'])


def flat(c):
    return levels_to_flat(c['cls']), levels_to_flat(c['reg']), levels_to_flat(c['soft'])


def prepare(c, cls, raw, scales, soft=None, soft_scales=None, ld=True, asg=None, soft_pad=4):
    """Assignment + quality pass (test_gfl_gpu.run_quality) of an LD plan, the teacher's rows bound; the padding columns of the class
    logits and of the teacher's rows (row stride 4R + soft_pad) hold NaN: they must not be read.  asg: labels / targets written over
    the device's own assignment (a synthetic placement of the positives)."""
    from dsl_amd.head_loss import FcosLossPlan
    plan = FcosLossPlan(c['B'], c['sizes'], 'cuda', num_classes=c['C'], head=options(c, ld), max_gt=64)
    plan.set_targets(c['gts'], c['gls'], None, c['pads'])
    plan.assign()
    if asg is not None:
        plan.labels.copy_(asg['labels'])
        plan.bbox_targets.copy_(asg['targets'])
    cl = torch.full((plan.M, plan.LD_CLS), float('nan'))
    cl[:, :c['C']] = cls
    plan.bind_outputs(cl.cuda(), raw.contiguous().cuda(), scales.cuda())
    plan.quality()
    if ld:
        R4 = 4 * (c['reg_max'] + 1)
        sf = torch.full((plan.M, R4 + soft_pad), float('nan'))
        sf[:, :R4] = soft
        plan.bind_soft(sf.cuda(), R4 + soft_pad, soft_scales.cuda())
    torch.cuda.synchronize()
    return plan


def run_loss(c, cls, raw, scales, soft=None, soft_scales=None, ld=True, asg=None, inv_world=1.0, norm_scale=None, fill=None):
    plan = prepare(c, cls, raw, scales, soft, soft_scales, ld, asg)
    if norm_scale is not None:
        from dsl_amd import ops
        plan.norm2 = plan.stats * norm_scale
        ops.set_ptrs(plan.desc, norm=plan.norm2)
        plan.configure(inv_world=inv_world)
    if fill is not None:
        plan.g_rc.fill_(fill)
    plan.loss()
    torch.cuda.synchronize()
    return plan


def ref_loss(c, a, cls, raw, scales, soft, soft_scales, norm=None):
    x, r, s = (v.double().requires_grad_() for v in (cls, raw, scales))
    out = LR.loss(x, r, s, soft.double(), soft_scales.double(), a, c['sizes'], c['B'], norm=norm, **ld_kw(c))
    return x, r, s, out


def check_loss(c, cls, raw, scales, soft, soft_scales, asg=None):
    """The bars of tests/test_gfl_gpu.py:85-111 (check_loss) against ld_ref's float64 autograd: losses rel 1e-4 / abs 1e-6 - loss_ld at
    the DFL term's bar, the same -, bf16 gradients 2^-8 of the entry + 2^-8 * 0.05 of the largest, g_scales rtol 1e-3 / atol 1e-6."""
    plan = run_loss(c, cls, raw, scales, soft, soft_scales, asg=asg)
    a = asg if asg is not None else ref_assign(c)
    assert torch.equal(plan.labels.cpu(), a['labels'])
    norm = None
    if asg is not None:          # stats[0] is the device assignment's, the weight sum the quality pass's over the placed positives
        wsum = GR.quality(cls.double(), raw.double(), scales.double(), a, c['sizes'], c['B'], c['reg_max'], c['C'])[2]
        norm = (float(plan.stats[0].cpu()), float(wsum))
        assert float(plan.stats[1].cpu()) == pytest.approx(float(wsum), rel=1e-5)
    x, r, s, (lc, lb, ldf, lld, _) = ref_loss(c, a, cls, raw, scales, soft, soft_scales, norm)
    total = lc + lb + ldf + lld
    total.backward()
    got, lv = plan.losses.cpu(), plan.logvec.cpu()
    assert len(lv) == 5
    for i, (k, v) in enumerate((('loss_cls', lc), ('loss_bbox', lb), ('loss_dfl', ldf), ('loss_ld', lld))):
        print(k, float(got[i]), float(v.detach()))
        assert float(got[i]) == pytest.approx(float(v.detach()), rel=1e-4, abs=1e-6), k
        assert float(lv[i]) == float(got[i])
    assert float(lv[4]) == pytest.approx(float(total.detach()), rel=1e-4, abs=1e-6)
    tol = 2 ** -8
    C, R4 = c['C'], 4 * (c['reg_max'] + 1)
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    for mine, ref in ((mine_c[:, :C], x.grad.float()), (mine_r[:, :R4], r.grad.float())):
        print('max |grad err|', float((mine - ref).abs().max()), 'of', float(ref.abs().max()))
        assert torch.allclose(mine, ref, rtol=tol, atol=tol * float(ref.abs().max()) * 0.05 + 1e-9)
    assert float(mine_c[:, C:].abs().max()) == 0.0
    if plan.LD_GRC > R4:
        assert float(mine_r[:, R4:].abs().max()) == 0.0
    assert torch.allclose(plan.g_scales.cpu()[:5], s.grad.float(), rtol=1e-3, atol=1e-6)
    off = (a['labels'] >= C).nonzero().view(-1)
    assert float(mine_r[off].abs().max()) == 0.0
    return plan, a


def check_ld_part_of_g_rc(c, cls, raw, scales, soft, soft_scales):
    """With the box and DFL weights at 0 the row's gradient is the LD term's alone: held to the same bf16 bar."""
    c0 = dict(c, bbox_weight=0.0, dfl_weight=0.0)
    plan = run_loss(c0, cls, raw, scales, soft, soft_scales)
    a = ref_assign(c0)
    x, r, s, (lc, lb, ldf, lld, _) = ref_loss(c0, a, cls, raw, scales, soft, soft_scales)
    assert float(lb) == 0.0 and float(ldf) == 0.0 and float(lld) > 0
    lld.backward()
    tol, R4 = 2 ** -8, 4 * (c['reg_max'] + 1)
    mine, ref = plan.g_rc.float().cpu()[:, :R4], r.grad.float()
    print('LD part: max |grad err|', float((mine - ref).abs().max()), 'of', float(ref.abs().max()))
    assert float(ref.abs().max()) > 0 and torch.allclose(mine, ref, rtol=tol, atol=tol * float(ref.abs().max()) * 0.05 + 1e-9)
    assert torch.allclose(plan.g_scales.cpu()[:5], s.grad.float(), rtol=1e-3, atol=1e-6)
    got = plan.losses.cpu()
    assert float(got[1]) == 0.0 and float(got[2]) == 0.0 and float(got[3]) == pytest.approx(float(lld), rel=1e-4, abs=1e-6)


@pytest.mark.parametrize('case', ['a', 'c', 'd'])
def test_loss_and_gradients_vs_float64(golden, case):
    """a: 80 classes, 68 box logits, T 10, teacher scales unlike the student's; c: 64 logits (one tile), T 1; d: reg_max 3, T 2.5,
    weight 1."""
    c = load_case(golden(f'ld_{case}.npz'))
    cls, raw, soft = flat(c)
    plan, _ = check_loss(c, cls, raw, c['scales'], soft, c['soft_scales'])
    assert (plan.LD_RC, plan.LD_GRC) == {'a': (68, 128), 'c': (64, 64), 'd': (16, 64)}[case] and float(plan.losses[3].cpu()) > 0.1
    check_ld_part_of_g_rc(c, cls, raw, c['scales'], soft, c['soft_scales'])
    again = run_loss(c, cls, raw, c['scales'], soft, c['soft_scales'])
    for u, v in ((plan.losses, again.losses), (plan.g_cls, again.g_cls), (plan.g_rc, again.g_rc), (plan.g_scales, again.g_scales)):
        assert torch.equal(u, v)


def test_one_class(golden):
    """Case a's arrays with a single class (the partial class group of the QFL pass beside the LD rows)."""
    c = load_case(golden('ld_a.npz'))
    cls, raw, soft = flat(c)
    c['C'], c['gls'] = 1, [torch.zeros_like(g) for g in c['gls']]
    check_loss(c, cls[:, :1].contiguous(), raw, c['scales'], soft, c['soft_scales'])


def last_wavefront_assignment(a, c):
    """Case a's positives (label, target box) placed on the locations of the last wavefront of each level - the 64-location chunks
    that hold a level's last location (9, 12 and the partial 13 of 856 locations), every other location background."""
    M, ends, e = a['labels'].numel(), [], 0
    for h, w in c['sizes']:
        e += c['B'] * h * w
        ends.append(e)
    chunks = sorted({(e - 1) // 64 for e in ends})
    slots = torch.tensor([m for ch in chunks for m in range(ch * 64, min(ch * 64 + 64, M))])
    pos = (a['labels'] < c['C']).nonzero().view(-1)
    k = min(len(slots), len(pos))
    labels, targets = torch.full_like(a['labels'], c['C']), torch.zeros_like(a['targets'])
    labels[slots[:k]], targets[slots[:k]] = a['labels'][pos[:k]], a['targets'][pos[:k]]
    assert chunks == [9, 12, 13] and k >= 128
    return dict(a, labels=labels, targets=targets)


def test_positives_in_the_last_wavefront_of_each_level(golden):
    c = load_case(golden('ld_a.npz'))
    cls, raw, soft = flat(c)
    asg = last_wavefront_assignment(ref_assign(c), c)
    plan, _ = check_loss(c, cls, raw, c['scales'], soft, c['soft_scales'], asg=asg)
    assert float(plan.losses[3].cpu()) > 0.1


def test_image_without_positives_and_batch_without_boxes(golden):
    c = load_case(golden('ld_b.npz'))
    cls, raw, soft = flat(c)
    plan, a = check_loss(c, cls, raw, c['scales'], soft, c['soft_scales'])
    assert a['npos'][1] == 0 and plan.npos.tolist() == a['npos'] and float(plan.losses[3].cpu()) > 0
    assert bool(torch.isfinite(plan.losses).all()) and bool(torch.isfinite(plan.g_rc.float()).all())
    c['gts'], c['gls'] = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    plan = run_loss(c, cls, raw, c['scales'], soft, c['soft_scales'], fill=1.0)          # (the gradient buffer full of ones)
    got = plan.losses.cpu()
    assert plan.npos.tolist() == [0, 0] and float(got[3]) == 0.0 and float(got[1]) == 0.0 and float(got[2]) == 0.0 and float(got[0]) > 0
    assert float(plan.g_rc.float().abs().max()) == 0.0 and bool(torch.isfinite(plan.g_cls.float()).all())
    assert float(plan.logvec[3].cpu()) == 0.0 and float(plan.logvec[4].cpu()) == float(got[0])


def test_zero_weight_equals_gfl_loss_bit_for_bit(golden):
    c = load_case(golden('ld_a.npz'))
    cls, raw, soft = flat(c)
    gfl = run_loss(c, cls, raw, c['scales'], ld=False)
    zero = run_loss(dict(c, ld_weight=0.0), cls, raw, c['scales'], soft, c['soft_scales'])
    assert gfl.ld is None and zero.ld is not None and zero.ld.w_ld == 0.0
    assert torch.equal(gfl.losses[:3], zero.losses[:3]) and float(zero.losses[3].cpu()) == 0.0 and float(gfl.losses[3].cpu()) == 0.0
    for u, v in ((gfl.g_cls, zero.g_cls), (gfl.g_rc, zero.g_rc), (gfl.g_scales, zero.g_scales)):
        assert torch.equal(u.view(torch.int16) if u.dtype == torch.bfloat16 else u.view(torch.int32),
                           v.view(torch.int16) if v.dtype == torch.bfloat16 else v.view(torch.int32))
    assert torch.equal(gfl.logvec[:3], zero.logvec[:3]) and float(gfl.logvec[3].cpu()) == float(zero.logvec[4].cpu())


@pytest.mark.parametrize('case', ['a', 'c'])
def test_teacher_equal_to_student_adds_nothing(golden, case):
    c = load_case(golden(f'ld_{case}.npz'))
    cls, raw, _ = flat(c)
    same = run_loss(c, cls, raw, c['scales'], raw, c['scales'])
    zero = run_loss(dict(c, ld_weight=0.0), cls, raw, c['scales'], raw, c['scales'])
    print('loss_ld', float(same.losses[3].cpu()))
    assert abs(float(same.losses[3].cpu())) <= 1e-6
    assert torch.equal(same.g_rc.view(torch.int16), zero.g_rc.view(torch.int16)) and torch.equal(same.g_cls.view(torch.int16), zero.g_cls.view(torch.int16))


def test_teacher_target_that_underflows(golden):
    """T = 1 (case c) and teacher rows with a logit gap of 120: exp(-120) is 0 in fp32, the term counts as 0 (F.kl_div), everything
    stays finite and loss_ld is float64's within the DFL bar."""
    c = load_case(golden('ld_c.npz'))
    cls, raw, soft = flat(c)
    a = ref_assign(c)
    pos = (a['labels'] < c['C']).nonzero().view(-1)
    soft = soft.clone()
    R = c['reg_max'] + 1
    rows = soft[pos[::2]].reshape(-1, 4, R)
    rows[:, :, 3], rows[:, :, 11] = 60.0, -60.0
    soft[pos[::2]] = rows.reshape(-1, 4 * R)
    ones = torch.ones(5)
    plan = run_loss(c, cls, raw, c['scales'], soft, ones)
    assert c['T'] == 1.0 and bool(torch.isfinite(plan.losses).all()) and bool(torch.isfinite(plan.g_rc.float()).all())
    assert bool(torch.isfinite(plan.g_scales).all())
    check_loss(c, cls, raw, c['scales'], soft, ones)


def test_two_ranks_with_doubled_sums_reproduce_one_rank(golden):
    """test_gfl_gpu.test_two_ranks_with_doubled_sums_reproduce_one_rank with the fourth term, which has no normaliser: unchanged."""
    c = load_case(golden('ld_d.npz'))
    cls, raw, soft = flat(c)
    one = run_loss(c, cls, raw, c['scales'], soft, c['soft_scales'])
    two = run_loss(c, cls, raw, c['scales'], soft, c['soft_scales'], inv_world=0.5, norm_scale=2.0)
    assert float(one.losses[3].cpu()) > 0.1
    for u, v in ((one.losses, two.losses), (one.g_cls, two.g_cls), (one.g_rc, two.g_rc), (one.g_scales, two.g_scales), (one.logvec, two.logvec)):
        assert torch.equal(u, v)


def test_wrong_descriptors_are_refused_and_launch_nothing(golden):
    from dsl_amd import _lib as L
    from dsl_amd.engine import OpList
    c = load_case(golden('ld_d.npz'))
    cls, raw, soft = flat(c)
    plan = prepare(c, cls, raw, c['scales'], soft, c['soft_scales'])
    plan.g_rc.fill_(3.0)
    plan.g_cls.fill_(3.0)
    plan.losses.fill_(7.0)
    ld, flags, keep = plan.ld, plan.desc.head_flags, (plan.ld.soft, plan.ld.soft_scales)
    nan, inf = float('nan'), float('inf')

    def refused(word, **kw):
        old = {k: getattr(ld, k) for k in kw}
        for k, v in kw.items():
            setattr(ld, k, v)
        with pytest.raises(RuntimeError, match=word):
            plan.loss()
        for k, v in old.items():
            setattr(ld, k, v)

    refused('soft', soft=None)
    refused('soft', soft_scales=None)
    refused('ld_soft', ld_soft=4 * (c['reg_max'] + 1) - 1)
    for t in (0.5, 0.0, -2.0, inf, nan):
        refused('T must be finite and >= 1', T=t)
    for w in (-0.25, inf, nan):
        refused('w_ld must be finite and >= 0', w_ld=w)
    assert (ld.soft, ld.soft_scales) == keep
    for bad in (flags & ~L.HEAD_GFL, flags & ~L.HEAD_LD):          # DSL_HEAD_LD without DSL_HEAD_GFL; a dsl_ld_desc without DSL_HEAD_LD
        plan.desc.head_flags = bad
        with pytest.raises(RuntimeError, match='DSL_HEAD_LD'):
            plan.loss()
    # the op list dispatches on DSL_HEAD_LD: without DSL_HEAD_GFL it reaches dsl_ld_loss, which refuses
    plan.desc.head_flags = flags & ~L.HEAD_GFL
    ol = OpList()
    ol.loss(plan.desc)
    with pytest.raises(RuntimeError, match='DSL_HEAD_LD'):
        ol.run()
    plan.desc.head_flags = flags
    plan.gfl.reg_max = 17          # ... and what dsl_gfl_loss refuses
    with pytest.raises(RuntimeError, match='dsl_ld_loss: reg_max'):
        plan.loss()
    plan.gfl.reg_max = c['reg_max']
    torch.cuda.synchronize()
    assert bool((plan.g_rc.float() == 3.0).all()) and bool((plan.g_cls.float() == 3.0).all()) and bool((plan.losses == 7.0).all())
    ol.run()          # the restored descriptor through the op list: dsl_ld_loss
    torch.cuda.synchronize()
    fresh = run_loss(c, cls, raw, c['scales'], soft, c['soft_scales'])
    assert torch.equal(plan.losses, fresh.losses) and torch.equal(plan.g_rc, fresh.g_rc) and float(plan.losses[3].cpu()) > 0.1


# ---- the model ------------------------------------------------------------------------------------------------------------------
TEACHER_SCALES = (1.25, 0.875, 1.125, 0.75, 1.0)


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """A GFL, an FCOS and an ATSS model's step before a distillation detector exists in the process, then that detector - student
    gfl_model_cfg() with LDHead, teacher a second gfl_model_cfg() with other seeds and Scale values - after ONE iteration of
    train_detector (configs/ld's optimizer) with the step's log record."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config, build_detector
    from test_atss_cpu import atss_model_cfg
    from util import fcos_model_cfg
    batch = make_batch()
    others = {k: build_detector(cfg).cuda() for k, cfg in (('gfl', gfl_model_cfg()), ('fcos', fcos_model_cfg()), ('atss', atss_model_cfg()))}
    before = {k: one_step(m, batch) for k, m in others.items()}
    work = str(tmp_path_factory.mktemp('ld'))
    model = build_detector(ld_model_cfg())
    ts = model.teacher_model.store
    ts.init_reference_style(7)
    ts.tview('head.scales')[:5].copy_(torch.tensor(TEACHER_SCALES))
    ts.dirty = True
    cfg = Config(dict(
        model=ld_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001), optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001, step=[8, 11]),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=work))
    start = model.store.train.clone()
    t_train, t_frozen = ts.train.clone(), ts.frozen.clone()
    runner = train_detector(model, [OneBatch(batch)], cfg, distributed=False, validate=False)
    torch.cuda.synchronize()
    recs = [json.loads(line) for line in open(os.path.join(work, 'train.log.json')) if 'loss' in line]
    return dict(model=model, batch=batch, rec=recs[-1], runner=runner, start=start, others=others, before=before,
                t_train=t_train, t_frozen=t_frozen)


def test_one_training_step_vs_reference_model(trained):
    """The logged losses against ld_ref evaluated on the device's own student and teacher logits: rel 3e-3
    (test_gfl_gpu.test_one_training_step_vs_reference_model's bar)."""
    model, batch, rec = trained['model'], trained['batch'], trained['rec']
    assert trained['runner'].iter == 1
    assert set(k for k in rec if k.startswith('loss')) == {'loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld', 'loss'}
    ts = model.teacher_model.store
    plans = list(model._engine.plans.values())
    plan = [p for p in plans if p.training and p.store is model.store][0]
    tplan = [p for p in plans if p.store is ts]
    assert len(tplan) == 1 and not tplan[0].training and not hasattr(tplan[0], 'lossplan')          # the teacher owns no training plan
    assert model.teacher_model._engine is None and not [p for p in plans if p.training and p.store is ts]
    tplan = tplan[0]
    lp = plan.lossplan
    assert lp.ld is not None and lp.ld.soft == tplan.bufs['regctr'].data_ptr() and lp.ld.ld_soft == 68
    assert lp.ld.soft_scales == ts.t32_ptr('head.scales') and (lp.ld.T, lp.ld.w_ld) == (10.0, 0.25)
    sizes = [tuple(s) for s in plan.level_sizes]
    assert sizes == AR.SIZES
    pads = [m['pad_shape'][:2] for m in batch['img_metas']]
    a = AR.assign(sizes, batch['gt_bboxes'], batch['gt_labels'], pads)
    assert torch.equal(lp.labels.cpu(), a['labels']) and min(a['npos']) > 0
    logits, rc, soft = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu(), tplan.bufs['regctr'].cpu()
    assert tuple(rc.shape) == (plan.M, 68) == tuple(soft.shape) and not torch.equal(rc, soft)
    scales = torch.ones(5)            # the step's forward pass ran with the student's initial Scale parameters
    lc, lb, ldf, lld, _ = LR.loss(logits[:, :80].double(), rc.double(), scales.double(), soft.double(), torch.tensor(TEACHER_SCALES).double(),
                                  a, sizes, 2)
    for k, v in (('loss_cls', lc), ('loss_bbox', lb), ('loss_dfl', ldf), ('loss_ld', lld)):
        print(k, rec[k], float(v))
        assert rec[k] == pytest.approx(float(v), rel=3e-3), k
    assert rec['loss'] == pytest.approx(float(lc + lb + ldf + lld), rel=3e-3) and rec['loss_ld'] > 0
    # the teacher is bit-identical, the student moved
    assert torch.equal(ts.train.cpu().view(torch.int32), trained['t_train'].cpu().view(torch.int32))
    assert torch.equal(ts.frozen.cpu().view(torch.int32), trained['t_frozen'].cpu().view(torch.int32))
    st = model.store
    assert bool(torch.isfinite(st.train).all())
    for name in ('head.cls_w', 'head.regctr_w', 'head.scales', 'bbox_head.reg_convs.0.conv.weight'):
        off, n, _ = st.train_regions[name]
        assert not torch.equal(st.train[off:off + n].cpu(), trained['start'][off:off + n].cpu()), name
    assert st.device.type == 'cuda' and ts.device.type == 'cuda'          # .cuda() moved the teacher too


def test_ld_gradient_reaches_the_student(trained):
    """The same student stepped with loss_ld's weight at 0 gives other box-predictor gradients: the LD term is in the backward pass."""
    from dsl_amd.registry import build_detector
    model, batch = trained['model'], trained['batch']
    losses, grad = one_step(model, batch)
    assert set(losses) == {'loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld'} and losses['loss_ld'] > 0
    again, grad2 = one_step(model, batch)
    assert again == losses and torch.equal(grad, grad2)
    off, n, _ = model.store.train_regions['head.regctr_w']
    plain = build_detector(gfl_model_cfg()).cuda()
    plain.load_state_dict(model.state_dict())
    pl, pg = one_step(plain, batch)
    assert {k: losses[k] for k in pl} == pl          # the three GFL terms are the GFL model's, bit for bit
    assert not torch.equal(grad[off:off + n], pg[off:off + n])
    oc, nc, _ = model.store.train_regions['head.cls_w']
    assert torch.equal(grad[oc:oc + nc], pg[oc:oc + nc])          # ... and the class predictor, which loss_ld does not reach, too


def test_other_models_beside_the_ld_model(trained):
    """test_gfl_gpu.test_fcos_and_atss_steps_beside_a_gfl_model's pattern: a GFL, an FCOS and an ATSS model give, after the distillation
    detector was built and trained in the same process, the bits they gave before it."""
    batch = trained['batch']
    for k, m in trained['others'].items():
        losses, grad = one_step(m, batch)
        assert losses == trained['before'][k][0] and torch.equal(grad, trained['before'][k][1]), k
    assert set(trained['before']['gfl'][0]) == {'loss_cls', 'loss_bbox', 'loss_dfl'}
    plan = [p for p in trained['others']['gfl']._engine.plans.values() if p.training][0]
    assert plan.lossplan.ld is None and len(plan.lossplan.logvec) == 4


def test_inference_is_the_students_alone(trained):
    from dsl_amd.registry import build_detector
    import numpy as np
    model, batch = trained['model'], trained['batch']
    plain = build_detector(gfl_model_cfg()).cuda()
    plain.load_state_dict(model.state_dict())
    for m in (model, plain):          # (a low threshold, so that the hardly trained model's scores around the 0.01 prior give boxes)
        m.test_cfg = dict(m.test_cfg, score_thr=0.001)
    got = model.simple_test(batch['img'], batch['img_metas'], rescale=False)
    want = plain.simple_test(batch['img'], batch['img_metas'], rescale=False)
    assert len(got) == 2 and all(sum(len(x) for x in r) > 0 for r in got)
    for g, w in zip(got, want):
        assert len(g) == len(w) == 80 and all(np.array_equal(x, y) for x, y in zip(g, w))
