"""PAA on the GPU: dsl_paa_assign / _pos_loss / _reassign against what the reference's own PAAHead and sklearn computed
(tests/golden/paa_*.npz), dsl_paa_loss against tests/paa_ref.py's float64 autograd (pinned to the reference by test_paa_cpu.py),
detection with score voting against tests/golden/paa_det_*.npz, one training step through train_detector, and two ranks."""
import json
import os

import numpy as np
import pytest
import torch

import paa_ref as PR
from test_paa_cpu import BAD_SAMPLES, CASES, load_case, paa_model_cfg, ref_assign, ref_loss, ref_reassign

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def options(c):
    from dsl_amd.params import HeadOptions
    return HeadOptions(head_kind='paa', atss_topk=c['topk'], anchor_scale=c['anchor_scale'], delta_stds=c['stds'], pos_iou_thr=c['thr'],
                       bbox_weight=c['bbox_weight'], cls_weight=c['cls_weight'], ctr_weight=c['iou_weight'])


def assigned_plan(c, max_gt=64):
    """A loss plan with the head outputs bound (the logits' padding columns hold NaN: they must not be read) and the first assignment run."""
    from dsl_amd.head_loss import FcosLossPlan
    plan = FcosLossPlan(c['B'], c['sizes'], 'cuda', num_classes=c['C'], head=options(c), max_gt=max_gt)
    plan.set_targets(c['gts'], c['gls'], None, c['pads'])
    C, M = c['C'], plan.M
    cl = torch.full((M, plan.LD_CLS), float('nan'))
    cl[:, :C] = c['cls']
    rc = torch.full((M, 8), float('nan'))
    rc[:, :4], rc[:, 4] = c['reg'], c['iou']
    plan.bind_outputs(cl.cuda(), rc.cuda(), c['scales'].cuda())
    plan._keep = (cl, rc)
    plan.assign()
    return plan


def refined_plan(c, d, feed=True):
    """... then dsl_paa_pos_loss and dsl_paa_reassign; feed: the reassignment reads the FIXTURE's pos_loss bits."""
    from dsl_amd import _lib as L
    import ctypes as C
    plan = assigned_plan(c)
    L.check(L.lib.dsl_paa_pos_loss(C.byref(plan.paa), L.stream_ptr()), 'dsl_paa_pos_loss')
    plan.own_pos_loss = plan.pos_loss.clone()
    if feed:
        plan.pos_loss.copy_(T(d['pos_loss']).cuda())
    L.check(L.lib.dsl_paa_reassign(C.byref(plan.paa), L.stream_ptr()), 'dsl_paa_reassign')
    torch.cuda.synchronize()
    return plan


def state(plan):
    return [t.cpu().clone() for t in (plan.labels, plan.cand_gt, plan.assign_idx, plan.cls_weight, plan.bbox_targets, plan.pos_weight,
                                      plan.npos, plan.stats, plan.pos_loss, plan.iou_target, plan.gmm_iters, plan.gmm_flags)]


@pytest.mark.parametrize('case', CASES)
def test_assign_bit_exact_vs_reference(golden, case):
    d = golden(f'paa_{case}.npz')
    c = load_case(d)
    plan = assigned_plan(c)
    torch.cuda.synchronize()
    got = state(plan)
    assert torch.equal(got[0], T(d['labels0']).long()) and torch.equal(got[1], T(d['cand_gt']).int()) and torch.equal(got[2], got[1])
    assert torch.equal(got[3], T(d['cls_weight']).float()) and torch.equal(got[4], T(d['targets']))
    assert bool((got[5] == 1).all()) and got[6].tolist() == [0, 0] and float(got[7].abs().max()) == 0.0
    if case == 'e':
        assert int((got[3] == 0).sum()) > 0 and bool((got[1][got[3] == 0] == -1).all())      # invalid anchors take no part
    again = assigned_plan(c)
    plan.assign()
    torch.cuda.synchronize()
    for p in (again, plan):
        assert all(torch.equal(a, b) for a, b in zip(got[:8], state(p)[:8]))


@pytest.mark.parametrize('case', ['a', 'e', 'f'])
def test_pos_loss_vs_reference(golden, case):
    d = golden(f'paa_{case}.npz')
    c = load_case(d)
    plan = refined_plan(c, d)
    got, want = plan.own_pos_loss.cpu(), T(d['pos_loss'])
    cand = T(d['cand_gt']) >= 0
    rel = ((got - want).abs() / want.clamp(min=1e-12))[cand]
    print('pos_loss: largest relative deviation', float(rel.max()), 'over', int(cand.sum()), 'candidates')
    assert float(rel.max()) <= 1e-5 and float(got[~cand].abs().max()) == 0.0 and int(cand.sum()) > 50


@pytest.mark.parametrize('case', CASES)
def test_reassign_on_the_fixture_losses(golden, case):
    d = golden(f'paa_{case}.npz')
    c = load_case(d)
    plan = refined_plan(c, d)
    got = state(plan)
    nb = len(d['box_n'])
    assert torch.equal(got[0], T(d['labels']).long()) and got[6].tolist() == [int(v) for v in d['npos']]
    assert got[10][:nb].tolist() == [int(v) for v in d['box_iter']] and got[11][:nb].tolist() == [int(v) for v in d['box_flag']]
    assert float(got[10][nb:].abs().max()) == 0 and float(got[11][nb:].abs().max()) == 0
    pos = got[0] < c['C']
    assert torch.equal(got[2] >= 0, pos) and torch.equal(got[2][pos], got[1][pos])          # assign_idx: the box of a kept anchor, else -1
    assert torch.equal(got[5] == 1, pos | (got[1] < 0)) and torch.equal(got[3], T(d['cls_weight']).float())      # box weight 0 where demoted
    want = T(d['iou_target'])
    print('iou_target: largest deviation', float((got[9] - want).abs().max()), 'sum', float(got[7][1]), float(want.double().sum()))
    assert torch.allclose(got[9], want, rtol=1e-5, atol=1e-6)
    assert float(got[7][0]) == float(sum(d['npos'])) and float(got[7][1]) == pytest.approx(float(want.double().sum()), rel=1e-5, abs=1e-6)
    assert float(got[7][2:].abs().max()) == 0.0
    if case == 'g':
        assert 1 in got[11][:nb].tolist()
    # the same over the used buffers: the reassignment reads nothing it wrote
    from dsl_amd import _lib as L
    import ctypes as C
    L.check(L.lib.dsl_paa_reassign(C.byref(plan.paa), L.stream_ptr()), 'dsl_paa_reassign')
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, state(plan)))


def test_ill_defined_covariance_gives_flag_2_and_a_finite_loss(golden):
    """One box's candidates get the losses BAD_SAMPLES[0] (one of them) and BAD_SAMPLES[1] (all others), for which paa_ref - like
    sklearn - finds a non-positive variance: flag 2, no positive for that box, every other box as before, a finite loss."""
    from dsl_amd import _lib as L
    import ctypes as C
    d = golden('paa_w.npz')
    c = load_case(d)
    plan = refined_plan(c, d)
    before = state(plan)
    g = int(np.argmax(d['box_n']))
    img, box = int(d['box_image'][g]), int(d['box_box'][g])
    ms = PR.mstarts(c['sizes'], c['B'])
    mine = torch.zeros(plan.M, dtype=torch.bool)
    for l, (h, w) in enumerate(c['sizes']):
        lo = int(ms[l]) + img * h * w
        mine[lo:lo + h * w] = T(d['cand_gt'])[lo:lo + h * w] == box
    idx = mine.nonzero().view(-1)
    pl = T(d['pos_loss']).clone()
    pl[idx] = BAD_SAMPLES[1]
    pl[idx[0]] = BAD_SAMPLES[0]
    a = ref_assign(c)
    re = ref_reassign(c, a, pl.numpy())
    assert re['boxes'][g]['flag'] == 2 and len(re['boxes'][g]['index']) >= 2
    plan.assign()
    L.check(L.lib.dsl_paa_pos_loss(C.byref(plan.paa), L.stream_ptr()), 'dsl_paa_pos_loss')      # (the ordered pair: iou_target afresh)
    plan.pos_loss.copy_(pl.cuda())
    L.check(L.lib.dsl_paa_reassign(C.byref(plan.paa), L.stream_ptr()), 'dsl_paa_reassign')
    plan.loss()
    torch.cuda.synchronize()
    got = state(plan)
    assert int(got[11][g]) == 2 and int(got[10][g]) == re['boxes'][g]['n_iter'] and got[11].tolist().count(2) == 1
    assert bool((got[0][idx] == c['C']).all()) and torch.equal(got[0], re['labels']) and got[6].tolist() == re['npos']
    assert torch.equal(got[0][~mine], before[0][~mine]) and torch.equal(got[9][~mine], before[9][~mine]) and float(got[9][mine].abs().max()) == 0.0
    assert bool(torch.isfinite(plan.losses).all()) and bool(torch.isfinite(plan.g_cls.float()).all()) and bool(torch.isfinite(plan.g_rc.float()).all())


def check_loss(c, d, plan):
    """test_atss_gpu.check_loss's bars against paa_ref's float64 autograd, on the reassignment of the fixture's losses."""
    a = ref_assign(c)
    re = ref_reassign(c, a, d['pos_loss'])
    assert torch.equal(plan.labels.cpu(), re['labels'])
    x, r, t, s = (v.double().requires_grad_() for v in (c['cls'], c['reg'], c['iou'], c['scales']))
    lc, lb, li, _ = ref_loss(c, a, re, x, r, t, s)
    (lc + lb + li).backward()
    got = plan.losses.cpu()
    for i, (k, v) in enumerate((('loss_cls', lc), ('loss_bbox', lb), ('loss_iou', li))):
        print(k, float(got[i]), float(v.detach()), float(d[k]) if k in d else '')
        assert float(got[i]) == pytest.approx(float(v.detach()), rel=1e-4, abs=1e-6), k
    assert float(got[3]) == 0.0 and plan.logvec.numel() == 4
    assert float(plan.logvec[3].cpu()) == pytest.approx(float(lc + lb + li), rel=1e-4, abs=1e-6)
    tol = 2 ** -8
    C = c['C']
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    zero = torch.zeros(plan.M)
    for mine, ref in ((mine_c[:, :C], x.grad.float()), (mine_r[:, :4], r.grad.float() if r.grad is not None else zero[:, None].expand(-1, 4)),
                      (mine_r[:, 4], t.grad.float() if t.grad is not None else zero)):
        print('max |grad err|', float((mine - ref).abs().max()), 'of', float(ref.abs().max()))
        assert torch.allclose(mine, ref, rtol=tol, atol=tol * float(ref.abs().max()) * 0.05 + 1e-9)
    assert float(mine_c[:, C:].abs().max()) == 0.0 and float(mine_r[:, 5:].abs().max()) == 0.0          # padding columns
    sgrad = s.grad.float() if s.grad is not None else torch.zeros(5)
    assert torch.allclose(plan.g_scales.cpu()[:5], sgrad, rtol=1e-3, atol=1e-6)
    return re


@pytest.mark.parametrize('case', ['a', 'e', 'f', 'n'])
def test_loss_and_gradients_vs_float64(golden, case):
    """a: 80 classes; e: invalid anchors (weight 0); f: 18 classes (the partial class group), topk 3; n: no box - loss_cls over
    max(num_pos, n) = 2, zero box terms and gradients."""
    d = golden(f'paa_{case}.npz')
    c = load_case(d)
    plan = refined_plan(c, d)
    plan.loss()
    torch.cuda.synchronize()
    re = check_loss(c, d, plan)
    if case == 'n':
        assert sum(re['npos']) == 0 and float(plan.losses[1]) == 0.0 and float(plan.losses[2]) == 0.0
        assert float(plan.g_rc.float().abs().max()) == 0.0 and float(plan.losses[0]) > 0
    if case == 'e':
        inv = (T(d['cls_weight']) == 0).nonzero().view(-1)
        assert len(inv) and float(plan.g_cls.float().cpu()[inv].abs().max()) == 0.0
    keep = [t.clone() for t in (plan.losses, plan.g_cls, plan.g_rc, plan.g_scales)]
    plan.loss()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(keep, (plan.losses, plan.g_cls, plan.g_rc, plan.g_scales)))


def test_whole_chain_on_the_wide_margin_case(golden):
    """assign -> pos_loss -> reassign -> loss with the kernels' own losses on case w (margins far above fp32 noise): the reference's
    labels exactly, its losses to 1e-3; and a second run is bit-identical."""
    d = golden('paa_w.npz')
    c = load_case(d)
    runs = []
    for _ in range(2):
        plan = refined_plan(c, d, feed=False)
        plan.loss()
        torch.cuda.synchronize()
        runs.append(state(plan) + [t.cpu().clone() for t in (plan.losses, plan.g_cls, plan.g_rc, plan.g_scales, plan.logvec)])
    got = runs[0]
    assert torch.equal(got[0], T(d['labels']).long()) and got[6].tolist() == [int(v) for v in d['npos']]
    assert got[10][:len(d['box_iter'])].tolist() == [int(v) for v in d['box_iter']]
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_iou')):
        print(k, float(got[12][i]), float(d[k]))
        assert float(got[12][i]) == pytest.approx(float(d[k]), rel=1e-3), k
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    # the op-list form of the middle pair gives the same bits
    from dsl_amd import _lib as L
    from dsl_amd.engine import OpList
    plan = assigned_plan(c)
    ol = OpList()
    ol.head_middle(L.OP_PAA_REFINE, plan.paa)
    ol.loss(plan.desc)
    ol.run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(runs[0][:12], state(plan))) and torch.equal(plan.losses.cpu(), runs[0][12])


def test_refused_descriptors_name_the_field(golden):
    from dsl_amd import _lib as L
    import ctypes as C
    c = load_case(golden('paa_b.npz'))
    plan = assigned_plan(c)
    q = plan.paa

    def refused(entry, word):
        rc = getattr(L.lib, entry)(C.byref(q), L.stream_ptr())
        assert rc != 0 and word in L.lib.dsl_last_error().decode(), (entry, word, L.lib.dsl_last_error())
    for field, bad, word in (('pos_iou_thr', 0.0, 'pos_iou_thr'), ('pos_iou_thr', 1.0, 'pos_iou_thr'), ('pos_loss', None, 'pos_loss'),
                             ('iou_target', None, 'iou_target'), ('cand_gt', None, 'cand_gt'), ('gmm_iters', None, 'gmm_iters'),
                             ('gmm_flags', None, 'gmm_flags')):
        old = getattr(q, field)
        setattr(q, field, bad)
        for entry in ('dsl_paa_assign', 'dsl_paa_pos_loss', 'dsl_paa_reassign', 'dsl_paa_loss'):
            refused(entry, word)
        setattr(q, field, old)
    old = plan.atss.topk
    plan.atss.topk = 17
    refused('dsl_paa_reassign', 'topk')
    plan.atss.topk = old
    flags = plan.desc.head_flags
    plan.desc.head_flags = flags & ~L.HEAD_PAA
    refused('dsl_paa_assign', 'head_flags')
    plan.desc.head_flags = flags
    assert L.lib.dsl_fcos_loss(C.byref(plan.desc), L.stream_ptr()) != 0 and 'dsl_paa_loss' in L.lib.dsl_last_error().decode()
    assert L.lib.dsl_atss_assign(C.byref(plan.desc), C.byref(plan.atss), L.stream_ptr()) != 0
    plan.assign()          # the descriptor is whole again
    torch.cuda.synchronize()


# ---- detection ------------------------------------------------------------------------------------------------------------------
def det_plan(d, score_voting):
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import DetectPlan
    from util import levels_to_flat
    C = int(d['num_classes'])
    cls, raw, iou = ([T(d[f'{k}{l}']) for l in range(5)] for k in ('cls', 'reg', 'iou'))
    ld = (C + 3) // 4 * 4
    flat = levels_to_flat(cls)
    cf = torch.full((flat.shape[0], ld), 30.0)
    cf[:, :C] = flat
    rc = torch.zeros(flat.shape[0], 8)
    rc[:, :4], rc[:, 4] = levels_to_flat(raw), levels_to_flat(iou)[:, 0]
    o = HeadOptions(head_kind='paa', score_voting=score_voting)
    dp = DetectPlan(2, PR.SIZES, PR.STRIDES, 'cuda', num_classes=C, nms_pre=int(d['nms_pre']), ld_cls=ld, iou_thr=float(d['iou_thr']),
                    score_thr=float(d['score_thr']), max_per_img=int(d['max_per_img']), head=o)
    dp.bind(cf.cuda(), rc.cuda(), T(d['scales']).cuda())
    dp.set_meta([tuple(s) for s in d['shapes']], [d['scale_factors'][i] for i in range(2)], True)
    dp.run()
    torch.cuda.synchronize()
    return dp


@pytest.mark.parametrize('name', 'ab')
def test_detect_with_score_voting_vs_reference(golden, name):
    """The reference's detections, labels and scores (scores to 1e-5), in its order; the voted boxes within 4 x the largest deviation
    of the reference's own fp32 boxes from paa_ref's float64 voting on this fixture (vote_dev, stored in the npz)."""
    d = golden(f'paa_det_{name}.npz')
    dp = det_plan(d, True)
    bar = 4.0 * float(d['vote_dev'])
    assert 1e-5 < bar < 1e-3
    for i in range(2):
        want, wl = d[f'dets{i}'], d[f'labels{i}']
        k = int(dp.count[i])
        got, gl = dp.dets[i, :k].cpu().numpy(), dp.labels[i, :k].cpu().numpy()
        assert k == len(want) and np.array_equal(gl, wl)
        assert np.abs(got[:, 4] - want[:, 4]).max() <= 1e-5
        dev = float(np.abs(got[:, :4].astype(np.float64) - want[:, :4]).max())
        print(f'paa_det_{name} image {i}: {k} detections, largest voted-box deviation {dev:.3e}, bar {bar:.3e}')
        assert dev <= bar
        assert float(np.abs(want[:, :4] - d[f'unvoted{i}']).max()) > 0.05      # (the vote moves boxes by far more than the bar)
    # voting off: the plain NMS output, i.e. the unvoted boxes in the NMS's own order
    plain = det_plan(d, False)
    for i in range(2):
        k = int(plain.count[i])
        got, gl = plain.dets[i, :k].cpu().numpy(), plain.labels[i, :k].cpu().numpy()
        assert k == int(dp.count[i]) and bool((np.diff(got[:, 4]) <= 0).all())
        order = np.argsort(gl, kind='stable')
        # (the reference's decoded boxes to test_num_classes_gpu._match's bars: the device's expf is not torch's bit for bit)
        assert np.array_equal(gl[order], d[f'labels{i}']) and np.allclose(got[order, :4], d[f'unvoted{i}'], rtol=1e-4, atol=1e-3)
        assert np.abs(got[order, 4] - d[f'dets{i}'][:, 4]).max() <= 1e-5


def test_tta_collect_refuses_a_paa_descriptor(golden):
    from dsl_amd.sweep import AugMerge
    dp = det_plan(golden('paa_det_b.npz'), True)
    mg = AugMerge(1, 5, 'cuda', num_classes=3, nms_pre=100, iou_thr=0.6)
    dp.n = 1
    dp.desc.n = 1
    with pytest.raises(RuntimeError, match='DSL_HEAD_PAA'):
        mg.collect(0, dp, (128, 160, 3), np.ones(4, np.float32), False, None)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """The PAA model after ONE iteration of train_detector (configs/paa's optimizer), with the step's log record."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config, build_detector
    from test_atss_gpu import OneBatch, make_batch
    work = str(tmp_path_factory.mktemp('paa'))
    model = build_detector(paa_model_cfg())
    cfg = Config(dict(
        model=paa_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2),
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
    """The logged losses against paa_ref evaluated on the device's own logits (the reassignment on the device's own candidate
    losses, which are compared first): rel 3e-3, test_atss_gpu.test_one_training_step_vs_reference_model's bar."""
    model, batch, rec = trained['model'], trained['batch'], trained['rec']
    assert trained['runner'].iter == 1 and set(k for k in rec if k.startswith('loss')) == {'loss_cls', 'loss_bbox', 'loss_iou', 'loss'}
    plan = [p for p in model._engine.plans.values() if p.training][0]
    lp = plan.lossplan
    assert lp.paa is not None and lp.atss is not None
    sizes = [tuple(s) for s in plan.level_sizes]
    assert sizes == PR.SIZES
    pads = [m['pad_shape'][:2] for m in batch['img_metas']]
    a = PR.assign(sizes, batch['gt_bboxes'], batch['gt_labels'], pads)
    assert torch.equal(lp.cand_gt.cpu(), a['cand_gt']) and torch.equal(lp.cls_weight.cpu(), a['cls_weight'])
    logits, rc = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu()
    scales = torch.ones(5)            # the step's forward pass ran with the initial Scale parameters
    pl = PR.pos_loss(logits[:, :80], rc[:, :4], scales, a, sizes, 2, 80, bbox_weight=1.3)
    mine = lp.pos_loss.cpu()
    assert torch.allclose(mine.double(), pl, rtol=1e-5, atol=0)
    re = PR.reassign(mine.numpy(), a, sizes, 2, [len(b) for b in batch['gt_bboxes']], 9, 80)
    assert torch.equal(lp.labels.cpu(), re['labels']) and lp.npos.tolist() == re['npos'] and sum(re['npos']) > 0
    nb = len(re['boxes'])
    assert lp.gmm_iters[:nb].tolist() == [b['n_iter'] for b in re['boxes']] and lp.gmm_flags[:nb].tolist() == [b['flag'] for b in re['boxes']]
    lc, lb, li, _ = PR.loss(logits[:, :80], rc[:, :4], rc[:, 4], scales, a, re, sizes, 2, 80, bbox_weight=1.3, iou_weight=0.5)
    for k, v in (('loss_cls', lc), ('loss_bbox', lb), ('loss_iou', li)):
        print(k, rec[k], float(v))
        assert rec[k] == pytest.approx(float(v), rel=3e-3), k
    assert rec['loss'] == pytest.approx(float(lc + lb + li), rel=3e-3)
    st = model.store
    assert bool(torch.isfinite(st.train).all())
    for name in ('head.cls_w', 'head.regctr_w', 'head.scales', 'bbox_head.reg_convs.0.conv.weight'):
        off, n, _ = st.train_regions[name]
        assert not torch.equal(st.train[off:off + n].cpu(), trained['before'][off:off + n].cpu()), name


def test_simple_test_runs_and_aug_test_raises(trained):
    model, batch = trained['model'], trained['batch']
    res = model.simple_test(batch['img'], batch['img_metas'], rescale=False)
    assert len(res) == 2 and all(len(r) == 80 for r in res)
    got = np.concatenate(res[0])
    assert np.isfinite(got).all()
    views = [batch['img'][:1], batch['img'][:1].flip(3)]
    metas = [[dict(batch['img_metas'][0])], [dict(batch['img_metas'][0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='PAA'):
        model.aug_test(views, metas, rescale=True)


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
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
    return build_detector(paa_model_cfg()).cuda()


def _rank_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from dsl_amd.parallel import HipDistributedDataParallel
        model = _build_cuda()
        ddp = HipDistributedDataParallel(model)
        out = ddp.train_step(_half(rank), None)
        torch.cuda.synchronize()
        logs = {k: float(v) for k, v in out['log_vars'].items()}
        lp = [p for p in model._engine.plans.values() if p.training][0].lossplan
        own = lp.losses.cpu().tolist()[:3]
        dist.destroy_process_group()
        q.put((rank, 'ok', logs, own))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None, None))


def test_two_ranks_exchange_no_normaliser(tmp_path):
    """World size 2 on one GPU (gloo): each rank's losses are the single-process losses of its own half - no normaliser crossed the
    ranks (paa_head.py:173-193 has no reduce_mean) - and the logged values are their mean."""
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
    single = []
    for rank in range(2):
        model = _build_cuda()
        out = model.train_step(_half(rank), None)
        torch.cuda.synchronize()
        single.append({k: float(v) for k, v in out['log_vars'].items()})
    keys = ('loss_cls', 'loss_bbox', 'loss_iou')
    for rank in range(2):
        for i, k in enumerate(keys):
            print(rank, k, res[rank][3][i], single[rank][k])
            assert res[rank][3][i] == pytest.approx(single[rank][k], rel=1e-5), (rank, k)
    assert abs(single[0]['loss_bbox'] - single[1]['loss_bbox']) > 1e-3 * single[0]['loss_bbox']      # the halves do differ
    for k in keys + ('loss',):
        assert res[0][2][k] == pytest.approx(0.5 * (single[0][k] + single[1][k]), rel=1e-5), k
        assert res[1][2][k] == pytest.approx(res[0][2][k], rel=1e-6)
