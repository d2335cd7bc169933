"""FoveaBox on the GPU: dsl_fovea_assign against the reference's own targets (tests/golden/fovea_*.npz) and, off the fixture geometry,
against tests/fovea_ref.py (pinned to the reference by test_fovea_cpu.py); dsl_fovea_loss and the DSL_HEAD_FOVEA detection against
fovea_ref; what the ABI refuses; one training step through train_detector, two ranks, and the other heads' plans beside a Fovea model."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import fovea_cases as FC
import fovea_ref as FR
from test_fovea_cpu import CASES, fovea_model_cfg, load_case, ref_loss

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def options(c):
    from dsl_amd.params import HeadOptions
    return HeadOptions(head_kind='fovea', sigma=c['sigma'], base_edge_list=c['base'], scale_ranges=c['ranges'], smooth_l1_beta=c['beta'],
                       focal_gamma=c['gamma'], focal_alpha=c['alpha'], cls_weight=c.get('cls_weight', 1.0), bbox_weight=c.get('bbox_weight', 1.0))


def assigned_plan(c, max_gt=128):
    from dsl_amd.head_loss import FcosLossPlan
    plan = FcosLossPlan(c.get('B', c.get('n')), c['sizes'], 'cuda', num_classes=c['C'], head=options(c), max_gt=max_gt)
    plan.set_targets(c['gts'], c['gls'])
    plan.assign()
    return plan


def assign_outputs(p):
    torch.cuda.synchronize()
    return [t.cpu().clone() for t in (p.labels, p.assign_idx, p.cls_weight, p.pos_weight, p.stats, p.bbox_targets)]


def check_assign(plan, a, n):
    """labels, assign_idx, the weights and stats exact; the log targets 1e-6 absolute at positives (four fp32 ulps at log 16: logf is
    the device library's), exactly 0 elsewhere."""
    lab, idx, cw, pw, st, tg = assign_outputs(plan)
    assert torch.equal(lab, a['labels']) and torch.equal(idx, a['assign_idx'])
    assert bool((cw == 1).all()) and bool((pw == 1).all())
    assert st.tolist() == [float(a['num_pos'] + n), float(max(a['num_pos'], 1)), 0, 0, 0, 0, 0, 0]
    pos = lab < plan.num_classes
    if bool(pos.any()):
        err = float((tg[pos] - a['targets'][pos]).abs().max())
        print('max |log target err|', err)
        assert err <= 1e-6
    assert not bool(tg[~pos].any())
    return lab, idx, cw, pw, st, tg


# ---- 1. the assignment against the fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_assign_vs_reference(case):
    c = load_case(case)
    d = c['d']
    plan = assigned_plan(c)
    got = check_assign(plan, dict(labels=T(d['labels']), assign_idx=T(d['assign_idx']), num_pos=int(d['num_pos']), targets=c['asg']['targets']), c['B'])
    pos = T(d['pos'])
    if len(pos):
        assert float((got[5][pos] - T(d['log_targets'])).abs().max()) <= 1e-6          # the reference's own log targets
    # a fresh plan and a rerun over the used workspace give the same bits
    again = assigned_plan(c)
    plan.assign()
    for p in (again, plan):
        assert all(torch.equal(u, v) for u, v in zip(got, assign_outputs(p)))


# ---- 2. the loss against fovea_ref in float64 ------------------------------------------------------------------------------------
def run_loss(c, cls, raw, plan=None):
    """Assignment + loss on flat level-major head outputs; the logits' padding columns hold NaN (they must not be read)."""
    plan = plan or assigned_plan(c)
    M = plan.M
    cl = torch.full((M, plan.LD_CLS), float('nan'))
    cl[:, :c['C']] = cls
    rc = torch.full((M, 8), float('nan'))
    rc[:, :4] = raw
    plan.bind_outputs(cl.cuda(), rc.cuda(), None)
    plan.loss()
    torch.cuda.synchronize()
    return plan


def check_loss(plan, C, lc, lb, gc, gr):
    """tests/test_atss_gpu.py::check_loss's bars: losses rel 1e-4 / abs 1e-6, gradients 2^-8 relative to the bf16 storage."""
    got = plan.losses.cpu()
    for i, (k, v) in enumerate((('loss_cls', lc), ('loss_bbox', lb))):
        print(k, float(got[i]), v)
        assert float(got[i]) == pytest.approx(v, rel=1e-4, abs=1e-6), k
    assert got[2:].tolist() == [0.0, 0.0]
    lv = plan.logvec.cpu()
    assert lv.shape == (3,) and lv[:2].tolist() == got[:2].tolist() and float(lv[2]) == pytest.approx(lc + lb, rel=1e-4, abs=1e-6)
    tol = 2 ** -8
    mine_c, mine_r = plan.g_cls.float().cpu(), plan.g_rc.float().cpu()
    for mine, ref in ((mine_c[:, :C], gc.float()), (mine_r[:, :4], gr.float())):
        print('max |grad err|', float((mine - ref).abs().max()), 'of', float(ref.abs().max()))
        assert torch.allclose(mine, ref, rtol=tol, atol=tol * float(ref.abs().max()) * 0.05 + 1e-9)
    assert float(mine_c[:, C:].abs().max()) == 0.0 and float(mine_r[:, 4:].abs().max()) == 0.0          # padding columns
    assert bool(torch.isfinite(mine_c).all())


@pytest.mark.parametrize('case', ['a', 'c', 'e'])
def test_loss_and_gradients_vs_float64(case):
    """a: 80 classes, gamma 1.5 / alpha 0.4 / beta 0.11, both SmoothL1 branches; c: no positive; e: 18 classes (the partial class
    group), gamma 2, beta 1, loss weights 2 / 0.5."""
    c = load_case(case)
    cls, raw = FR.flat(c['cls']), FR.flat(c['reg'])
    plan = run_loss(c, cls, raw)
    assert torch.equal(plan.labels.cpu(), c['asg']['labels'])
    check_loss(plan, c['C'], *ref_loss(case))
    if case == 'c':
        assert float(plan.losses[1]) == 0.0 and not bool(plan.g_rc.any()) and plan.stats[:2].tolist() == [2.0, 1.0]
    again = run_loss(c, cls, raw)
    for u, v in ((plan.losses, again.losses), (plan.logvec, again.logvec), (plan.g_cls, again.g_cls), (plan.g_rc, again.g_rc)):
        assert torch.equal(u, v)


def test_grad_scale_scales_the_gradients_only():
    c = load_case('e')
    cls, raw = FR.flat(c['cls']), FR.flat(c['reg'])
    one = run_loss(c, cls, raw)
    plan = assigned_plan(c)
    plan.configure(grad_scale=0.25)
    run_loss(c, cls, raw, plan)
    assert torch.equal(plan.losses, one.losses)
    for u, v in ((plan.g_cls, one.g_cls), (plan.g_rc, one.g_rc)):          # (a power of two: exact in bf16)
        assert torch.equal(u.float(), v.float() * 0.25)


# ---- 3. generated cases off the fixture geometry ---------------------------------------------------------------------------------
def generated_loss_ref(c, a):
    cls, raw = c['cls'].double().requires_grad_(), c['raw'].double().requires_grad_()
    lc, lb = FR.loss(cls, raw, a, c['n'], c['C'], c['gamma'], c['alpha'], c['beta'])
    (lc + lb).backward()
    return float(lc.detach()), float(lb.detach()), cls.grad, raw.grad


def test_four_images_with_an_empty_one_and_a_level_of_twenty_workgroups():
    c, a = FC.case('four_images'), FC.ref('four_images')
    assert c['n'] * c['sizes'][0][0] * c['sizes'][0][1] == 20 * 256 and len(c['gts'][2]) == 0
    total = sum(len(b) for b in c['gts'])
    plan = assigned_plan(c, max_gt=total)          # max_gt boxes in the batch: the capacity is the only cap
    lab = check_assign(plan, a, c['n'])[0]
    M2 = [sum(h * w for h, w in c['sizes'][:l]) * c['n'] for l in range(6)]
    for l, (h, w) in enumerate(c['sizes']):          # the empty image is background on every level; its neighbours are not
        seg = lab[M2[l]:M2[l + 1]].reshape(c['n'], h * w)
        assert bool((seg[2] == c['C']).all())
    assert a['num_pos'] > 50
    run_loss(c, c['cls'], c['raw'], plan)
    check_loss(plan, c['C'], *generated_loss_ref(c, a))


def test_seventy_boxes_in_one_image_and_a_reused_plan_with_fewer():
    c, a = FC.case('many_boxes'), FC.ref('many_boxes')
    assert len(c['gts'][0]) == 70
    plan = assigned_plan(c)
    idx = check_assign(plan, a, c['n'])[1]
    assert int(idx.max()) >= 64          # a winner from the second LDS chunk
    run_loss(c, c['cls'], c['raw'], plan)
    check_loss(plan, c['C'], *generated_loss_ref(c, a))
    # the next step of the same plan has fewer boxes: nothing of the step before survives
    f, af = FC.case('fewer'), FC.ref('fewer')
    plan.set_targets(f['gts'], f['gls'])
    plan.assign()
    check_assign(plan, af, f['n'])
    assert af['num_pos'] < a['num_pos']
    run_loss(f, f['cls'], f['raw'], plan)
    check_loss(plan, f['C'], *generated_loss_ref(f, af))


# ---- 4. detection ----------------------------------------------------------------------------------------------------------------
DET_C, DET_SHAPES, DET_SF = 20, [(128, 160), (100, 130)], [1.0, 1.25]


def det_inputs(seed=5, shift=-2.0):
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(2, DET_C, h, w, generator=g) * 2.0 + shift for h, w in FR.SIZES]
    raw = [torch.randn(2, 4, h, w, generator=g) * 0.8 for h, w in FR.SIZES]
    return cls, raw


def det_plan(cls, raw, n=2, **kw):
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import DetectPlan
    flat = FR.flat(cls)
    cf = torch.full((flat.shape[0], DET_C), 30.0)
    cf[:, :DET_C] = flat
    rc = torch.full((flat.shape[0], 8), float('nan'))          # columns 4..7 are not read: no centerness
    rc[:, :4] = FR.flat(raw)
    dp = DetectPlan(n, [tuple(c.shape[2:]) for c in cls], FR.STRIDES, 'cuda', num_classes=DET_C, nms_pre=100, ld_cls=DET_C,
                    head=HeadOptions(head_kind='fovea'), **kw)
    dp.bind(cf.cuda(), rc.cuda(), None)
    return dp


@pytest.mark.parametrize('rescale', [False, True])
def test_detect_vs_reference_model(rescale):
    """dsl_fcos_detect with DSL_HEAD_FOVEA against fovea_ref.detect (its decode + the project's CPU NMS model), compared as
    tests/test_atss_gpu.py::test_detect_vs_reference_model compares (test_num_classes_gpu._match).  nms_pre 100 < level 0's 320
    locations; the second image is smaller than the canvas."""
    from test_num_classes_gpu import _match
    cls, raw = det_inputs()
    dp = det_plan(cls, raw)
    dp.set_meta(DET_SHAPES, DET_SF, rescale)
    dp.run()
    torch.cuda.synchronize()
    ref = FR.detect(cls, raw, DET_SHAPES, DET_SF if rescale else None, nms_pre=100)
    assert all(len(r[0]) >= 10 for r in ref)
    _match(dp.dets, dp.labels, dp.count, ref, 2)
    k = int(dp.count[1])
    b = dp.dets[1, :k, :4].cpu() * (1.25 if rescale else 1.0)
    assert float(b[:, [0, 2]].max()) == pytest.approx(129.0, abs=1e-3) and float(b[:, [1, 3]].max()) == pytest.approx(99.0, abs=1e-3)
    assert float(b.min()) >= 0.0


def test_detect_soft_nms_and_no_test_time_augmentation():
    import soft_nms_ref as S
    from dsl_amd import _lib as L
    from dsl_amd.sweep import AugMerge
    from test_num_classes_gpu import _match
    # (seed and shift chosen on the CPU model: every pick and the cut at max_per_img are decided by a relative score gap > 6e-4,
    # far above what the device's expf / sigmoid can move)
    cls, raw = det_inputs(12, -5.0)
    dp = det_plan(cls, raw, iou_thr=0.3, nms_method=L.NMS_LINEAR, soft_min_score=1e-3)
    dp.set_meta(DET_SHAPES, DET_SF, False)
    dp.run()
    torch.cuda.synchronize()
    ref = []
    for i in range(2):
        b, s, c = FR.collect([x[i:i + 1] for x in cls], [x[i:i + 1] for x in raw], DET_SHAPES[i], np.ones(4), 100)
        dets, labels, rec = S.soft_nms(*S.valid_pairs(b, s, c, 0.05), 0.3, 100, 'linear')
        e = rec['emitted']
        assert min(rec['pick_gaps']) > 5e-4 and (e[99] - e[100]) / e[99] > 5e-4 and rec['n_decays'] >= 5
        ref.append((dets, labels))
    _match(dp.dets, dp.labels, dp.count, ref, 2)
    # FoveaHead.get_bboxes has no with_nms argument: a view's collect refuses the flag
    one = det_plan([x[:1] for x in cls], [x[:1] for x in raw], n=1)
    mg = AugMerge(2, 5, 'cuda', num_classes=DET_C, nms_pre=100)
    with pytest.raises(RuntimeError, match='DSL_HEAD_FOVEA has no test-time augmentation'):
        mg.collect(0, one, (128, 160, 3), np.ones(4, np.float32))


# ---- 5. what the ABI refuses -----------------------------------------------------------------------------------------------------
def refused(fn, desc, match):
    from dsl_amd import _lib as L
    rc = getattr(L.lib, fn)(C.byref(desc), L.stream_ptr())
    msg = L.lib.dsl_last_error().decode()
    assert rc != 0 and match in msg, (fn, rc, msg)


def test_abi_refusals():
    from dsl_amd import _lib as L
    c = load_case('d')
    plan = run_loss(c, FR.flat(c['cls']), FR.flat(c['reg']))
    d, f = plan.desc, plan.fovea
    assert C.addressof(d) == C.addressof(f) and d.head_flags == L.HEAD_FOVEA | L.HEAD_LOSS_EXT
    keep = (d.head_flags, d.ig_boxes, d.ig_off, f.sigma, f.lo[1], f.smooth_l1_beta, d.workspace_bytes, d.soft_weight, d.loss_weight)
    d.ig_boxes, d.ig_off = plan.ig_boxes.data_ptr(), plan.ig_off.data_ptr()
    for fn in ('dsl_fovea_assign', 'dsl_fovea_loss', 'dsl_head_assign', 'dsl_head_loss'):
        refused(fn, d, 'ig_boxes')
    d.ig_boxes, d.ig_off = keep[1], keep[2]
    for extra in (L.HEAD_ATSS, L.HEAD_GFL, L.HEAD_PAA, L.HEAD_LD, L.HEAD_EXP_DECODE):
        d.head_flags = keep[0] | extra
        for fn in ('dsl_head_assign', 'dsl_head_loss'):
            refused(fn, d, 'head_flags')
    d.head_flags = L.HEAD_FOVEA          # without the loss family
    refused('dsl_fovea_loss', d, 'head_flags')
    d.head_flags = keep[0]
    refused('dsl_fcos_assign', d, 'DSL_HEAD_FOVEA')
    refused('dsl_fcos_loss', d, 'DSL_HEAD_FOVEA')
    for bad in (0.0, 1.5, -0.1, float('nan')):
        f.sigma = bad
        refused('dsl_fovea_assign', d, 'sigma')
    f.sigma = keep[3]
    f.lo[1] = f.hi[1] + 1.0
    refused('dsl_fovea_assign', d, 'lo[1] > hi[1]')
    f.lo[1] = keep[4]
    for bad in (0.0, -1.0):
        f.smooth_l1_beta = bad
        refused('dsl_fovea_loss', d, 'smooth_l1_beta')
    f.smooth_l1_beta = keep[5]
    d.workspace_bytes = keep[6] - 1
    refused('dsl_fovea_assign', d, 'workspace')
    refused('dsl_fovea_loss', d, 'workspace')
    d.workspace_bytes = keep[6]
    d.soft_weight = 0.5
    refused('dsl_fovea_loss', d, 'soft_weight')
    d.soft_weight = keep[7]
    d.loss_weight = 0.5
    refused('dsl_fovea_loss', d, 'loss_weight')
    d.loss_weight = keep[8]
    # restored: the descriptor runs again and gives the bits of before
    before = (plan.losses.clone(), plan.g_rc.clone(), plan.labels.clone())
    plan.assign()
    plan.loss()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(before, (plan.losses, plan.g_rc, plan.labels)))


# ---- 6. the model ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """The Fovea model after ONE iteration of train_detector (configs/foveabox's optimizer), with the step's log record."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.registry import Config, build_detector
    from test_atss_gpu import OneBatch, make_batch
    work = str(tmp_path_factory.mktemp('fovea'))
    torch.manual_seed(3)
    model = build_detector(fovea_model_cfg())
    cfg = Config(dict(
        model=fovea_model_cfg(), data=dict(samples_per_gpu=2, workers_per_gpu=2),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001), optimizer_config=dict(grad_clip=None),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001, step=[8, 11]),
        runner=dict(type='EpochBasedRunner', max_epochs=1), checkpoint_config=dict(interval=1000),
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]),
        log_level='ERROR', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=work))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batch = make_batch()
    runner = train_detector(model, [OneBatch(batch)], cfg, distributed=False, validate=False)
    torch.cuda.synchronize()
    recs = [json.loads(line) for line in open(os.path.join(work, 'train.log.json')) if 'loss' in line]
    return dict(model=model, batch=batch, rec=recs[-1], runner=runner, before=before)


def test_one_training_step(trained):
    """The logged losses are the loss kernel's, and fovea_ref's on the device's own head outputs (rel 3e-3,
    test_atss_gpu.test_one_training_step_vs_reference_model's bar); every trainable parameter moved."""
    model, batch, rec = trained['model'], trained['batch'], trained['rec']
    assert trained['runner'].iter == 1 and set(k for k in rec if k.startswith('loss')) == {'loss_cls', 'loss_bbox', 'loss'}
    plan = [p for p in model._engine.plans.values() if p.training][0]
    lp = plan.lossplan
    assert lp.fovea is not None and lp.atss is None and lp.kind.name == 'fovea'
    sizes = [tuple(s) for s in plan.level_sizes]
    assert sizes == FR.SIZES
    a = FR.assign(batch['gt_bboxes'], batch['gt_labels'], sizes, 80)
    assert torch.equal(lp.labels.cpu(), a['labels']) and torch.equal(lp.assign_idx.cpu(), a['assign_idx']) and a['num_pos'] > 0
    own = lp.losses.cpu().tolist()
    logits, rc = plan.bufs['cls_logits'].cpu(), plan.bufs['regctr'].cpu()
    assert rc.shape[1] == 8 and model.store.reg_rows == 4 and model.state_dict()['bbox_head.conv_reg.weight'].shape[0] == 4
    lc, lb = FR.loss(logits[:, :80].double(), rc[:, :4].double(), a, 2, 80, gamma=1.5, alpha=0.4, beta=0.11)
    for i, (k, v) in enumerate((('loss_cls', lc), ('loss_bbox', lb))):
        print(k, rec[k], own[i], float(v))
        assert rec[k] == pytest.approx(own[i], rel=1e-4, abs=1e-4), k          # (the text log keeps five decimals)
        assert own[i] == pytest.approx(float(v), rel=3e-3), k
    assert rec['loss'] == pytest.approx(own[0] + own[1], rel=1e-4, abs=1e-4)
    st = model.store
    assert bool(torch.isfinite(st.train).all())
    grads = st.named_views(st.grad)
    after = model.state_dict()
    same = [k for k in grads if torch.equal(after[k].cpu(), trained['before'][k].cpu())]
    assert not same, same


def test_state_dict_round_trip_simple_test_and_aug_test(trained):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    model, batch = trained['model'], trained['batch']
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert not any('scales' in k or 'centerness' in k for k in sd)
    other = build_detector(fovea_model_cfg()).cuda()
    other.load_state_dict(sd)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in other.state_dict().items())
    res = model.simple_test(batch['img'], batch['img_metas'], rescale=False)
    res2 = other.simple_test(batch['img'], batch['img_metas'], rescale=False)
    assert len(res) == 2 and all(len(r) == 80 and all(x.shape[1] == 5 and x.dtype == np.float32 for x in r) for r in res)
    assert all(np.array_equal(x, y) for r, r2 in zip(res, res2) for x, y in zip(r, r2))
    got = np.concatenate(res[1])
    assert np.isfinite(got).all() and (len(got) == 0 or (got[:, 2].max() <= 127 and got[:, 3].max() <= 95))          # img_shape (96, 128) - 1
    views = [batch['img'][:1], batch['img'][:1].flip(3)]
    metas = [[dict(batch['img_metas'][0])], [dict(batch['img_metas'][0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='FoveaHead does not support test-time augmentation'):
        model.aug_test(views, metas, rescale=True)


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
    return build_detector(fovea_model_cfg()).cuda()


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
        opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
        out = ddp.train_step(_half(rank), opt)
        out['loss'].backward()
        opt.step()
        model.store.wait_pending()
        torch.cuda.synchronize()
        lp = [p for p in model._engine.plans.values() if p.training][0].lossplan
        own = lp.losses.cpu().tolist()[:2]
        w = model.store.train.detach().cpu()
        lst = [torch.zeros_like(w) for _ in range(world)]
        dist.all_gather(lst, w)
        same = all(torch.equal(t, lst[0]) for t in lst)
        dist.destroy_process_group()
        q.put((rank, 'ok', same, own))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), False, None))


def test_two_ranks_end_with_identical_weights_and_exchange_no_statistics():
    """World size 2 on one GPU (gloo, as tests/test_ddp_gpu.py arranges it): each rank's losses are the single-process losses of its
    own half - no normaliser crossed the ranks (fovea_head.py:134-182 has no reduce_mean) - and after the optimizer step both ranks
    hold the same weights."""
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
    single = []
    for rank in range(2):
        model = _build_cuda()
        out = model.train_step(_half(rank), None)
        torch.cuda.synchronize()
        single.append([float(out['log_vars'][k]) for k in ('loss_cls', 'loss_bbox')])
    for rank in range(2):
        print(rank, res[rank][3], single[rank])
        assert res[rank][3] == pytest.approx(single[rank], rel=1e-5)
    assert abs(single[0][1] - single[1][1]) > 1e-3 * single[0][1]          # the halves do differ


# ---- 7. the new kind leaks into nothing ------------------------------------------------------------------------------------------
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
def test_plan_signature_beside_a_fovea_model(cfg_fn):
    before = _signature(cfg_fn)
    model = _build_cuda()
    plan = model._get_engine().plan(model.store, 2, 64, 96, training=True)
    assert plan.lossplan.kind.name == 'fovea'
    torch.cuda.synchronize()
    after = _signature(cfg_fn)
    assert len(before.splitlines()) > 100 and before == after
