"""Class counts other than 80 on the GPU: the fused loss (partial last group of 4 classes), whole training steps, the
optimizer / EMA on the padded classification predictor, the detection sweep (masked padding columns), the pseudo-label fuse
kernel, an RLA DSL iteration and train_detector on a VOC-shaped (20-class) configuration."""
import numpy as np
import pytest
import torch

from util import fcos_model_cfg, levels_to_flat, oracle_threads, rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy
STRIDES = (8, 16, 32, 64, 128)
PAD_FILL = 50.0          # padding columns of the logits: sigmoid(50) = 1 would win every max if it were read


def pads(C):
    return -(-C // 64) * 64, -(-C // 4) * 4


def build(C, rla=False, **head):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from oracle import fcos_oracle as O
    from oracle import rla_oracle as RO
    cfg = fcos_model_cfg(num_classes=C, **head)
    if rla:
        cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
    model = build_detector(cfg)
    model.load_state_dict((RO if rla else O).synth_state_dict(0, num_classes=C))
    return model.cuda()


# ---- fused loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3, 20])
def test_loss_vs_reference_golden(golden, C):
    """The bars of test_fcos_loss_gpu.test_loss_vs_reference_golden on the reference's C-class FCOSHead.loss (DSL batch of 3,
    sisoft on, ignore boxes); the logits' padding columns hold PAD_FILL, the gradient columns C .. round_up(C, 64) stay 0."""
    from dsl_amd.head_loss import FcosLossPlan
    d = golden(f'loss_c{C}.npz')
    assert int(d['num_classes']) == C
    B = int(d['B'])
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    cls = [T(d[f'cls{i}']) for i in range(5)]
    reg, ctr = [T(d[f'reg{i}']) for i in range(5)], [T(d[f'ctr{i}']) for i in range(5)]
    cp, c4 = pads(C)
    plan = FcosLossPlan(B, sizes, 'cuda', num_classes=C)
    assert (plan.LD_CLS, plan.LD_GCLS) == (c4, cp) and tuple(plan.g_cls.shape) == (plan.M, cp)
    plan.g_cls.fill_(3.0)                 # the kernel writes columns [0, c4): 0 in the tail lanes; the rest is the plan's zeros
    plan.g_cls[:, c4:] = 0
    plan.set_targets([T(d[f'gt{i}']) for i in range(B)], [T(d[f'gl{i}']) for i in range(B)], [T(d[f'ig{i}']) for i in range(B)])
    plan.configure(loss_weight=float(d['loss_weight']), soft_weight=float(d['soft_weight']) / 1000.0)   # inside the warm-up window
    cls_d = torch.full((plan.M, c4), PAD_FILL)
    cls_d[:, :C] = levels_to_flat(cls)
    rc = torch.zeros(plan.M, 8)
    rc[:, :4] = levels_to_flat(reg)
    rc[:, 4] = levels_to_flat(ctr)[:, 0]
    plan.bind_outputs(cls_d.cuda(), rc.cuda(), torch.ones(5, device='cuda'))
    plan.assign()
    plan.loss()
    torch.cuda.synchronize()
    got = plan.losses.cpu()
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft')):
        assert float(got[i]) == pytest.approx(float(d[k]), rel=1e-4, abs=1e-6), k
    gc = levels_to_flat([T(d[f'gcls{i}']) for i in range(5)])
    mine = plan.g_cls.float().cpu()
    assert float(mine[:, C:].abs().max()) == 0.0
    tol = 2 ** -8
    assert torch.allclose(mine[:, :C], gc, rtol=tol, atol=tol * float(gc.abs().max()) * 0.05 + 1e-9)
    gr = levels_to_flat([T(d[f'greg{i}']) for i in range(5)])
    on = levels_to_flat(reg) > 0
    assert torch.allclose(plan.g_rc.float().cpu()[:, :4][on], gr[on], rtol=tol, atol=tol * float(gr.abs().max()) * 0.05 + 1e-9)


# ---- whole training step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,B,H,W', [(20, 2, 608, 800), (3, 1, 480, 640)])
def test_train_step_vs_oracle(C, B, H, W):
    """The bars of test_step_gpu.test_train_step_vs_oracle_other_batch_sizes_and_shapes at C classes (VOC's size after resize and
    pad 32; a 3-class 640 x 480 batch of one)."""
    from oracle import fcos_oracle as O
    model = build(C)
    rng = np.random.RandomState(30 + C)
    g = torch.Generator().manual_seed(11 + C)
    img = (torch.randn(B, 3, H, W, generator=g) * 40).bfloat16().float()
    gtb = [T(O.synth_boxes(rng, 5, H=H, W=W, lo=16, hi=min(H, W))) for _ in range(B)]
    gtl = [T(rng.randint(0, C, len(b)).astype('int64')) for b in gtb]
    losses = model.forward_train(img.cuda(), [dict()] * B, gtb, gtl)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    got = {k: float(v.detach()) for k, v in losses.items()}
    plan = next(iter(model._engine.plans.values()))
    assert tuple(plan.bufs['cls_logits'].shape) == (plan.M, pads(C)[1])
    sd = O.synth_state_dict(0, num_classes=C)
    with oracle_threads():
        ol, og, aux = O.train_step(sd, img, gtb, gtl, None, emulate_bf16=True, num_classes=C)
        _, g32, _ = O.train_step(sd, img, gtb, gtl, None, emulate_bf16=False, num_classes=C)
    for k in got:
        assert got[k] == pytest.approx(ol[k], rel=3e-3), (k, got[k], ol[k])
    _, raux = O.fcos_loss([t.detach() for t in aux['cls']], [t.detach() for t in aux['reg']], [t.detach() for t in aux['ctr']],
                          gtb, gtl, None, num_classes=C, return_aux=True)
    assert torch.equal(plan.lossplan.labels.cpu(), raux['labels'])
    assert torch.equal(plan.lossplan.assign_idx.cpu().long(), raux['assign_idx'])
    named = dict(model.named_parameters())
    bad = []
    for k, gref in g32.items():
        if k not in named or named[k].grad is None or float(gref.norm()) == 0:
            continue
        e_hip, e_emu = rel_l2(named[k].grad.cpu(), gref), rel_l2(og[k], gref)
        if e_hip > 1.6 * e_emu + 5e-3:
            bad.append((k, float(e_hip), float(e_emu)))
    assert not bad, bad[:10]
    st = model.store
    assert float(st.tview('head.cls_w', st.grad)[C:].abs().max()) == 0.0
    assert float(st.tview('head.cls_b', st.grad)[C:].abs().max()) == 0.0


def test_sgd_clip_and_ema_keep_the_padding_rows_zero():
    """Three FlatSGD steps (momentum, weight decay, clip at 10) and one EMA update at 20 classes: the 44 padding rows of the
    classification predictor stay exactly 0 in the weights, gradients, momentum and teacher; the clip coefficient is the
    one of the unpadded gradients."""
    from dsl_amd.optim import FlatSGD
    from dsl_amd.runner import SemiEpochBasedRunner
    from oracle import fcos_oracle as O
    C = 20
    model, teacher = build(C), build(C)
    opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.),
                  grad_clip=dict(max_norm=10, norm_type=2))
    rng = np.random.RandomState(4)
    g = torch.Generator().manual_seed(4)
    st = model.store
    for it in range(3):
        img = torch.randn(2, 3, 96, 128, generator=g) * 40
        gtb = [T(O.synth_boxes(rng, 3, H=96, W=128, lo=8, hi=90)) for _ in range(2)]
        gtl = [T(rng.randint(0, C, len(b)).astype('int64')) for b in gtb]
        losses = model.forward_train(img.cuda(), [dict(img_shape=(96, 128, 3))] * 2, gtb, gtl)
        sum(losses.values()).backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
        coef_ref, norm_ref = O.clip_coef(grads, 10.0)
        norm = float(opt.gnorm_sq.cpu().sqrt())
        assert norm == pytest.approx(norm_ref, rel=1e-4)
        assert min(10.0 / (norm + 1e-6), 1.0) == pytest.approx(coef_ref, rel=1e-4)
        for name in ('head.cls_w', 'head.cls_b'):
            for buf in (st.train, st.grad, opt.momentum_buf):
                assert float(st.tview(name, buf)[C:].abs().max()) == 0.0, (it, name)
        assert float(st.train16[st.toff('head.cls_w'):st.toff('head.cls_w') + 64 * 2304].view(64, 2304)[C:].float().abs().max()) == 0
    runner = SemiEpochBasedRunner(model, optimizer=opt, max_epochs=1, ema_model=teacher)
    t0 = teacher.store.train.clone()
    runner.EMA(keep_rate=0.99)
    torch.cuda.synchronize()
    ts = teacher.store
    assert torch.allclose(ts.train, t0 * 0.99 + st.train * 0.01, rtol=1e-5, atol=1e-7)
    for name in ('head.cls_w', 'head.cls_b'):
        assert float(ts.tview(name)[C:].abs().max()) == 0.0


# ---- detection sweep ----------------------------------------------------------------------------------------------------
def _match(dets, labels, count, ref, n):
    """test_sweep_gpu._match against the oracle's (dets, labels) per image."""
    for i in range(n):
        k = int(count[i])
        rb, rl = ref[i][0], ref[i][1]
        assert k == rb.shape[0], (k, rb.shape)
        got_b, got_l = dets[i, :k].cpu(), labels[i, :k].cpu()
        assert torch.allclose(got_b[:, 4], rb[:, 4], rtol=1e-4, atol=1e-6)
        order_ref = np.lexsort((rb[:, 0].numpy(), rl.numpy(), -rb[:, 4].numpy()))
        order_got = np.lexsort((got_b[:, 0].numpy(), got_l.numpy(), -got_b[:, 4].numpy()))
        assert torch.equal(got_l[order_got], rl[order_ref])
        assert torch.allclose(got_b[order_got], rb[order_ref], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('C,ld', [(3, 4), (20, 20), (20, 24), (1, 4)])
def test_detect_vs_oracle(C, ld):
    """dsl_fcos_detect on identical logits vs the oracle's get_bboxes; the logit rows are `ld` wide and their padding columns
    hold PAD_FILL (the key kernel's max must not see them)."""
    from dsl_amd.sweep import DetectPlan
    from oracle import fcos_oracle as O
    sizes = [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)]
    B, shp = 2, (316, 444)
    g = torch.Generator().manual_seed(C + ld)
    cls = [torch.randn(B, C, h, w, generator=g) * 1.5 - 2.5 for h, w in sizes]
    reg = [torch.rand(B, 4, h, w, generator=g) * 6 * s for (h, w), s in zip(sizes, STRIDES)]
    ctr = [torch.randn(B, 1, h, w, generator=g) for h, w in sizes]
    flat = torch.full((sum(B * h * w for h, w in sizes), ld), PAD_FILL)
    flat[:, :C] = levels_to_flat(cls)
    rc = torch.zeros(flat.shape[0], 8)
    rc[:, :4] = levels_to_flat([r / s for r, s in zip(reg, STRIDES)])
    rc[:, 4] = levels_to_flat(ctr)[:, 0]
    dp = DetectPlan(B, sizes, STRIDES, 'cuda', num_classes=C, ld_cls=ld)
    dp.bind(flat.cuda(), rc.cuda(), torch.ones(5, device='cuda'))
    sf = np.array([1.25, 1.25, 1.25, 1.25], np.float32)
    dp.set_meta([shp] * B, [sf] * B, True)
    dp.run()
    torch.cuda.synchronize()
    ref = O.get_bboxes(cls, reg, ctr, [shp] * B, [sf.tolist()] * B)
    assert all(len(r[0]) > 0 for r in ref)
    _match(dp.dets, dp.labels, dp.count, ref, B)
    assert int(dp.labels.max()) < C


@pytest.mark.parametrize('C', [3, 20])
def test_simple_test_vs_oracle(C):
    """The whole sweep (bf16 network forward + detect) on a C-class model against the oracle's get_bboxes on the same weights:
    per class lists, and the confident reference detections found with near-identical boxes (test_sweep_gpu's criteria)."""
    from oracle import fcos_oracle as O
    model = build(C)
    sd = O.synth_state_dict(0, num_classes=C)
    g = torch.Generator().manual_seed(5)
    img = (torch.randn(2, 3, 128, 192, generator=g) * 40).bfloat16().float()
    shp = (128, 190, 3)
    metas = [dict(img_shape=shp, scale_factor=np.ones(4, np.float32))] * 2
    res = model.simple_test(img.cuda(), metas, rescale=True)
    assert len(res) == 2 and all(len(r) == C for r in res)
    with torch.no_grad():
        cls, reg, ctr = O.extract_and_head(sd, img, O.Quant(True), training=False)[:3]
    ref = O.get_bboxes(cls, reg, ctr, [shp] * 2, [[1.0] * 4] * 2)
    for i in range(2):
        got = np.concatenate(res[i])
        rb, rl = ref[i][0].numpy(), ref[i][1].numpy()
        assert abs(len(got) - len(rb)) <= max(2, len(rb) // 10), (len(got), len(rb))
        for c in range(C):
            assert res[i][c].shape[1] == 5
        for r, l in list(zip(rb[np.argsort(-rb[:, 4])], rl[np.argsort(-rb[:, 4])]))[:20]:
            cand = res[i][int(l)]
            assert len(cand), (l, r)
            dist = np.abs(cand[:, :4] - r[:4]).max(1)
            j = dist.argmin()
            assert dist[j] < 1.0 and abs(cand[j, 4] - r[4]) < 0.02, (r, cand[j])


# ---- pseudo-label fuse --------------------------------------------------------------------------------------------------
def test_fuse_kernel_20_classes_vs_host():
    from dsl_amd import _lib as L
    from dsl_amd.pseudo import fuse_host
    C, maxk, n = 20, 100, 3
    rng = np.random.RandomState(21)
    dets = np.zeros((n, maxk, 5), np.float32)
    labels = np.zeros((n, maxk), np.int64)
    counts = np.array([maxk, 37, 0], np.int32)
    for i in range(n):
        k = counts[i]
        base = rng.uniform(0, 400, (k, 2)).astype(np.float32)
        wh = rng.uniform(4, 120, (k, 2)).astype(np.float32)
        dets[i, :k, :2], dets[i, :k, 2:4] = base, base + wh
        dets[i, :k, 4] = rng.rand(k).astype(np.float32)
        labels[i, :k] = rng.randint(0, C, k)
        if k > 4:                      # near-duplicates of one class, so that the second NMS has work
            dets[i, 1:4] = dets[i, 0] + np.array([1.5, -0.5, 2.0, 1.0, -0.01], np.float32)
            labels[i, 1:4] = labels[i, 0]
    ob, osc = torch.empty(n, maxk, 4, device='cuda'), torch.empty(n, maxk, device='cuda')
    ol, oc = torch.empty(n, maxk, dtype=torch.int64, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
    dd, ld, cd = T(dets).cuda(), T(labels).cuda(), T(counts).cuda()
    L.check(L.lib.dsl_pseudo_label_fuse(L.ptr(dd), L.ptr(ld), L.ptr(cd), n, maxk, C, 0.2, 0.6, 0.1, L.ptr(ob), L.ptr(osc),
                                        L.ptr(ol), L.ptr(oc), L.stream_ptr()))
    torch.cuda.synchronize()
    for i in range(n):
        ref = fuse_host(dets[i, :counts[i]], labels[i, :counts[i]], 0.2, 0.6, 0.1, num_classes=C)
        k = int(oc[i])
        assert k == len(ref['tags'])
        assert ob[i, :k].cpu().numpy().tolist() == ref['rects'].tolist()
        assert ol[i, :k].cpu().tolist() == ref['tags'].tolist()
        assert osc[i, :k].cpu().numpy().tolist() == ref['scores'].tolist()


# ---- RLA DSL iteration --------------------------------------------------------------------------------------------------
def test_rla_dsl_iteration_vs_oracle():
    """RLA_ResNet, 20 classes, the semi-supervised batch of 3 (labeled, unlabeled with an ignore band, its half-scale copy),
    loss_weight 3, sisoft at full weight: the bars of test_rla_gpu.test_rla_train_step_vs_oracle."""
    from dsl_amd.runner import append_half_scale
    from oracle import fcos_oracle as O
    from oracle import rla_oracle as RO
    C = 20
    kw = dict(loss_weight=3.0, soft_weight=1.0)
    model = build(C, rla=True, soft_warm_up=0, **kw)
    model.bbox_head.cur_iter = 1                      # past the warm-up window
    rng = np.random.RandomState(8)
    g = torch.Generator().manual_seed(8)
    H, W = 128, 192
    img = (torch.randn(2, 3, H, W, generator=g) * 40).bfloat16().float()
    gtb = [T(O.synth_boxes(rng, 4, H=H, W=W, lo=8, hi=min(H, W))) for _ in range(2)]
    gtl = [T(rng.randint(0, C, len(b)).astype('int64')) for b in gtb]
    ig = [torch.zeros(0, 4), T(O.synth_boxes(rng, 3, H=H, W=W, lo=8, hi=100))]
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * 2
    oimg, ogb, ogl, ogi = O.append_half_scale(img, gtb, gtl, ig)
    _, _, _, _, metas3 = append_half_scale(img[:, :, :8, :8], gtb, gtl, ig, metas)
    losses = model.forward_train(oimg.cuda(), metas3, ogb, ogl, ogi)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert set(losses) == {'loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft'}
    got = {k: float(v.detach()) for k, v in losses.items()}
    sd = RO.synth_state_dict(0, num_classes=C)
    with oracle_threads():
        l32, g32, aux = RO.train_step(sd, oimg, ogb, ogl, ogi, emulate_bf16=False, soft_scale=1.0, num_classes=C, **kw)
        lem, gem, _ = RO.train_step(sd, oimg, ogb, ogl, ogi, emulate_bf16=True, soft_scale=1.0, num_classes=C, **kw)
    print('losses hip', got, 'oracle-bf16', lem, 'fp32', l32)
    for k in ('loss_cls', 'loss_bbox', 'loss_centerness'):
        assert got[k] == pytest.approx(lem[k], rel=3e-3), (k, got[k], lem[k])
        assert got[k] == pytest.approx(l32[k], rel=1e-3), (k, got[k], l32[k])
    # bf16 storage of the two logits adds a positive offset to every squared difference (test_rla_gpu's full-size DSL test); the
    # emulating oracle reproduces it.  On this small canvas it is +3.6e-3 relative against fp32, hence the bars 1e-3 / 1e-2
    assert got['loss_sisoft'] == pytest.approx(lem['loss_sisoft'], rel=1e-3)
    assert got['loss_sisoft'] == pytest.approx(l32['loss_sisoft'], rel=1e-2)
    plan = [p for p in model._engine.plans.values() if p.N == 3][0]
    _, raux = O.fcos_loss([t.detach() for t in aux['cls']], [t.detach() for t in aux['reg']], [t.detach() for t in aux['ctr']],
                          ogb, ogl, ogi, return_aux=True, soft_scale=1.0, num_classes=C, **kw)
    assert torch.equal(plan.lossplan.assign_idx.cpu().long(), raux['assign_idx'])
    assert torch.equal(plan.lossplan.labels.cpu(), raux['labels'])
    named = dict(model.named_parameters())
    tk = RO.trainable_keys(sd)
    bad, noisy = [], []
    for k in tk:
        e_hip, e_emu = rel_l2(named[k].grad.detach().cpu(), g32[k]), rel_l2(gem[k], g32[k])
        if e_emu > 0.25:
            noisy.append(k)
            continue
        if float(g32[k].norm()) > 0 and e_hip > 1.6 * e_emu + 5e-3:
            bad.append((k, e_hip, e_emu))
    assert not bad, bad[:10]
    assert len(noisy) <= 60, noisy
    for name in ('bbox_head.conv_cls.weight', 'bbox_head.conv_cls.bias'):
        assert tuple(named[name].shape)[0] == C
    st = model.store
    assert float(st.tview('head.cls_w', st.grad)[C:].abs().max()) == 0.0


# ---- train_detector on a VOC-shaped configuration -----------------------------------------------------------------------
def test_voc_config_trains_through_train_detector(tmp_path):
    """configs/fcos_semi/voc/RLA_*.py's sections (restated: the GPU box has no reference tree; tests/test_num_classes_cpu.py
    builds the real files): 20 classes, RLA_ResNet student + EMA teacher, clip 10, the synthetic semi-supervised loader on a
    20-class bank, teacher refresh + adathres, evaluation = dict(metric='mAP'); two short epochs."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.data import SyntheticSemiLoader, SyntheticValLoader
    from dsl_amd.pseudo import PseudoLabelBank
    from dsl_amd.registry import Config, build_detector
    C = 20
    model_cfg = fcos_model_cfg(num_classes=C, loss_weight=3.0, soft_weight=1.0, soft_warm_up=5000)
    model_cfg['backbone'] = dict(type='RLA_ResNet', layers=[3, 4, 6, 3], frozen_stages=1, norm_eval=True, style='pytorch')
    model_cfg['test_cfg'] = dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6),
                                 max_per_img=100)
    cfg = Config(dict(
        model=model_cfg,
        data=dict(samples_per_gpu=2, workers_per_gpu=2, batch_config=dict(ratio=[[1, 1]]),
                  unlabel_train=dict(thres='adathres.json'),
                  unlabel_pred=dict(type='SemiVOCDataset', num_gpus=1, infer_score_thre=0.1, first_score_thre=0.1, use_ema=True,
                                    eval_flip=False, fuse_history=False, first_fuse=False, eval_config={'iou': [0.6]},
                                    eval_checkpoint_config=dict(interval=1, mode='iteration'), preload=6, start_point=1)),
        optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.)),
        optimizer_config=dict(grad_clip=dict(max_norm=10, norm_type=2)),
        lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[40, 52]),
        runner=dict(type='SemiEpochBasedRunner', max_epochs=2), checkpoint_config=dict(interval=1),
        ema_config=dict(interval=1, mode='iteration', ratio=0.99, start_point=1), scale_invariant=True,
        log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]), custom_hooks=[dict(type='NumClassCheckHook')],
        log_level='WARNING', load_from=None, resume_from=None, workflow=[('train', 1)], work_dir=str(tmp_path)))
    student, teacher = build_detector(cfg.model), build_detector(cfg.model)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        student.init_weights()
        teacher.init_weights()
    bank = PseudoLabelBank(num_classes=C, thres='adathres.json')
    loader = SyntheticSemiLoader(bank, n_labeled=3, n_unlabeled=3, iters_per_epoch=3, H=128, W=192, W_img=190, img_std=30.0)
    assert len(loader.CLASSES) == C
    cfg.val_dataloader = SyntheticValLoader(n_images=2, num_classes=C, H=128, W=192, W_img=190)
    cfg.evaluation = dict(interval=1, metric='mAP')
    runner = train_detector(student, [loader], cfg, distributed=False, validate=True, ema_model=teacher)
    torch.cuda.synchronize()
    assert runner.iter == 6 and runner.epoch == 2 and runner.ema_flag
    assert torch.isfinite(student.store.train).all() and torch.isfinite(teacher.store.train).all()
    for store in (student.store, teacher.store):
        assert float(store.tview('head.cls_w')[C:].abs().max()) == 0.0
    import json
    import os
    recs = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'train.log.json'))]
    assert len(recs) == 6 and all('loss_cls' in r for r in recs)
    for r in recs:
        for k, v in r.items():
            if k.startswith('loss'):
                assert np.isfinite(v), (k, v)
    hook = [h for h in runner._hooks if type(h).__name__ == 'UnlabelPredHook'][0]
    assert hook.num_classes == C and hook.n_refreshed == 3 + 1
    assert all(int(t) < C for n in bank.names() for t in bank[n]['tags'])
    ev = [h for h in runner._hooks if type(h).__name__ == 'EvalHook'][0]
    assert [e for e, _ in ev.history] == [1, 2]
    for _, m in ev.history:
        assert set(m) == {'AP50', 'mAP'} and 0.0 <= m['mAP'] <= 1.0
    ck = torch.load(os.path.join(str(tmp_path), 'latest.pth'), map_location='cpu')
    assert tuple(ck['state_dict']['bbox_head.conv_cls.weight'].shape) == (C, 256, 3, 3)
