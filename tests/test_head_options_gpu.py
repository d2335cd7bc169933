"""FCOSHead options off the fcos_semi "tricks" head on the GPU: inside-box assignment, exp decode, IoU log loss, centerness on the
classification tower, bias-free towers - kernels against the reference's own outputs (tests/golden/make_golden_head_options.py),
the whole step against the reference and against tests/head_options_ref.py (pinned to the reference by test_head_options_cpu.py)."""
import numpy as np
import pytest
import torch

import head_options_ref as HR
from test_head_options_cpu import LOSS_LEGS, PLAIN_HEAD, load_loss_leg, opts_of
from util import fcos_model_cfg, levels_to_flat, oracle_threads, rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy
STRIDES = (8, 16, 32, 64, 128)


def head_options(o):
    from dsl_amd.params import HeadOptions
    return HeadOptions(**{k: bool(o[k]) for k in HeadOptions.FIELDS})


def build_plain(**head):
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    model = build_detector(fcos_model_cfg(**dict(PLAIN_HEAD, **head)))
    model.load_state_dict(HR.plain_state_dict(0))
    return model.cuda()


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('name', ['assign_plain_small.npz', 'assign_plain_full.npz'])
def test_inside_box_assign_bit_exact_vs_reference(golden, name, norm):
    from dsl_amd.head_loss import FcosLossPlan
    d = golden(name)
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    n = int(d['n_img'])
    plan = FcosLossPlan(n, sizes, 'cuda', head=head_options(HR.options(center_sampling=False, norm_on_bbox=norm)))
    plan.set_targets([T(d[f'gt{i}']) for i in range(n)], [T(d[f'gl{i}']) for i in range(n)], None)
    plan.assign()
    torch.cuda.synchronize()
    assert torch.equal(plan.labels.cpu(), T(d['labels']).long())
    assert torch.equal(plan.bbox_targets.cpu(), T(d['bbox_targets_norm_t' if norm else 'bbox_targets_t']).t())     # bit exact
    assert int(plan.stats[0]) == int((T(d['labels']) < 80).sum())


def run_leg(leg, reg=None):
    """The fixture's head outputs through assign + loss in the layout the engine uses for these options; the logits' padding
    columns hold NaN (they must not be read)."""
    from dsl_amd.head_loss import FcosLossPlan
    C = leg['C']
    plan = FcosLossPlan(leg['B'], leg['sizes'], 'cuda', num_classes=C, head=head_options(leg['opts']))
    plan.set_targets(leg['gtb'], leg['gtl'], leg['ig'])
    plan.configure(loss_weight=leg['loss_weight'], soft_weight=leg['soft_weight'] / 1000.0)
    plan.assign()                      # (before the outputs are bound, as the engine's multi-rank order does)
    M = plan.M
    cls = torch.full((M, plan.LD_CLS), float('nan'))
    cls[:, :C] = levels_to_flat(leg['cls'])
    rc = torch.zeros(M, 8)
    rc[:, :4] = levels_to_flat(leg['reg']) if reg is None else reg
    if plan.ctr_col is None:
        rc[:, 4] = levels_to_flat(leg['ctr'])[:, 0]
    else:
        cls[:, plan.ctr_col] = levels_to_flat(leg['ctr'])[:, 0]
        rc[:, 4] = float('nan')
    cls_d, rc_d, sc = cls.cuda(), rc.cuda(), leg['scales'].cuda()
    plan.bind_outputs(cls_d, rc_d, sc)
    plan.loss()
    torch.cuda.synchronize()
    return plan


def ctr_grad(plan):
    return (plan.g_rc[:, 4] if plan.ctr_col is None else plan.g_cls[:, plan.ctr_col]).float().cpu()


@pytest.mark.parametrize('name', LOSS_LEGS)
def test_loss_vs_reference_golden(golden, name):
    """The bars of test_fcos_loss_gpu.test_loss_vs_reference_golden: loss sums rel 1e-4 / abs 1e-6, bf16 gradients 2^-8 with the same
    absolute term, g_scales rtol 1e-3.  `greg` is the gradient w.r.t. the raw conv_reg output (through Scale and relu / exp)."""
    d = golden(name + '.npz')
    leg = load_loss_leg(d)
    plan = run_leg(leg)
    got = plan.losses.cpu()
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness', 'loss_sisoft')):
        if k in d.files:
            print(name, k, float(got[i]), float(d[k]))
            assert float(got[i]) == pytest.approx(float(d[k]), rel=1e-4, abs=1e-6), k
    gc = levels_to_flat([T(d[f'gcls{i}']) for i in range(5)])
    gr = levels_to_flat([T(d[f'greg{i}']) for i in range(5)])
    gt_ = levels_to_flat([T(d[f'gctr{i}']) for i in range(5)])[:, 0]
    tol = 2 ** -8
    C = leg['C']
    mine_c = plan.g_cls.float().cpu()
    assert torch.allclose(mine_c[:, :C], gc, rtol=tol, atol=tol * float(gc.abs().max()) * 0.05 + 1e-9)
    mine_r = plan.g_rc.float().cpu()
    assert torch.allclose(mine_r[:, :4], gr, rtol=tol, atol=tol * float(gr.abs().max()) * 0.05 + 1e-9)
    assert torch.allclose(ctr_grad(plan), gt_, rtol=tol, atol=tol * float(gt_.abs().max()) * 0.05 + 1e-9)
    if plan.ctr_col is None:
        assert float(mine_c[:, C:].abs().max()) == 0.0 and float(mine_r[:, 5:].abs().max()) == 0.0
    else:       # classes | zeros up to round_up(C, 4) | centerness | zeros
        assert plan.ctr_col == (C + 3) // 4 * 4 and float(mine_c[:, C:plan.ctr_col].abs().sum()) == 0.0
        assert float(mine_c[:, plan.ctr_col + 1:].abs().max()) == 0.0 and float(mine_r[:, 4:].abs().max()) == 0.0
    assert torch.allclose(plan.g_scales.cpu(), T(d['gscales']), rtol=1e-3, atol=1e-6)
    # run-to-run: the same bits
    again = run_leg(leg)
    for a, b in ((plan.losses, again.losses), (plan.g_cls, again.g_cls), (plan.g_rc, again.g_rc), (plan.g_scales, again.g_scales)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('case', ['clamp_active', 'iou_one', 'no_positives'])
def test_iou_loss_edges_vs_fp64(golden, case):
    """IoU log loss at its edges against the restatement in float64: a regression logit so large that clamp(iou, eps) is active (loss
    -log(eps), no gradient through the clamp), predictions equal to their targets (iou == 1: loss 0), and no positive location -
    finite gradients everywhere."""
    d = golden('loss_plain_nopos.npz' if case == 'no_positives' else 'loss_plain_sup.npz')
    leg = load_loss_leg(d)
    if case == 'iou_one':          # relu decode with power-of-two scales: raw * scale == target exactly
        leg['opts'] = HR.options(center_sampling=False, iou_loss=True)
        leg['scales'] = torch.tensor([1.0, 0.5, 2.0, 1.0, 0.25])
    o = leg['opts']
    from oracle import fcos_oracle as O
    labels, tg, _ = HR.get_targets(O.get_points(leg['sizes']), leg['gtb'], leg['gtl'], o)
    raw = levels_to_flat(leg['reg']).clone()
    # level-major flat order [lvl][img][y][x]: the reference's per-level concatenation over images
    fl, ft = torch.cat(labels), torch.cat(tg)
    lvl = torch.cat([torch.full((leg['B'] * h * w,), i) for i, (h, w) in enumerate(leg['sizes'])])
    pos = (fl < 80).nonzero().view(-1)
    if case == 'clamp_active':
        raw[pos[:8]] = 14.0            # exp(14 * scale): boxes of 10^4 .. 10^7 pixels, iou < 1e-6
    if case == 'iou_one':
        raw[pos[:8]] = ft[pos[:8]] / leg['scales'][lvl[pos[:8]]].view(-1, 1)
    plan = run_leg(leg, reg=raw)
    assert torch.equal(plan.labels.cpu(), fl)
    # float64 restatement on the same operands
    B = leg['B']
    split = lambda flat, c: [t.view(B, h, w, c).permute(0, 3, 1, 2) for t, (h, w) in zip(flat.split([B * h * w for h, w in leg['sizes']]), leg['sizes'])]
    r64 = raw.double().requires_grad_()
    sc64 = leg['scales'].double().requires_grad_()
    z = [r * sc64[i] for i, r in enumerate(split(r64, 4))]
    pred = [torch.relu(t) if o['norm_on_bbox'] else t.exp() for t in z]
    c64 = [c.double().requires_grad_() for c in leg['ctr']]
    out = HR.fcos_loss([c.double() for c in leg['cls']], pred, c64, [b.double() for b in leg['gtb']], leg['gtl'], None, opts=o)
    sum(out.values()).backward()
    got = plan.losses.cpu()
    print(case, 'loss_bbox', float(got[1]), float(out['loss_bbox']))
    assert float(got[1]) == pytest.approx(float(out['loss_bbox']), rel=1e-4, abs=1e-6)
    assert float(got[2]) == pytest.approx(float(out['loss_centerness']), rel=1e-4, abs=1e-6)
    g = plan.g_rc.float().cpu()[:, :4]
    assert torch.isfinite(g).all() and torch.isfinite(plan.g_cls.float()).all() and torch.isfinite(plan.g_scales).all()
    ref = r64.grad.float()
    assert torch.allclose(g, ref, rtol=2 ** -7, atol=2 ** -8 * float(ref.abs().max()) * 0.05 + 1e-9)
    assert torch.allclose(plan.g_scales.cpu(), sc64.grad.float(), rtol=1e-3, atol=1e-6)
    if case == 'clamp_active':
        assert float(g[pos[:8]].abs().max()) == 0.0 and float(ref[pos[:8]].abs().max()) == 0.0
    if case == 'no_positives':
        assert float(got[1]) == 0.0 and float(g.abs().max()) == 0.0 and int(plan.stats[0]) == 0


def test_detect_exp_decode_vs_reference(golden):
    """dsl_fcos_detect with the exp decode and the centerness logit in the classification predictor's column, on the reference's own
    head outputs, against the reference's get_bboxes (test_detect_vs_oracle's tolerances)."""
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import DetectPlan
    from test_num_classes_gpu import _match
    d = golden('sweep_tiny_plain.npz')
    cls, reg, ctr = ([T(d[f'{k}{i}']) for i in range(5)] for k in ('cls', 'reg', 'ctr'))
    sizes = [tuple(c.shape[-2:]) for c in cls]
    flat = torch.full((sum(2 * h * w for h, w in sizes), 84), 1e30)
    flat[:, :80] = levels_to_flat(cls)
    flat[:, 80] = levels_to_flat(ctr)[:, 0]
    rc = torch.zeros(flat.shape[0], 8)
    rc[:, :4] = levels_to_flat(reg).log()            # the fixture holds exp(scale * x)
    rc[:, 4] = 1e30
    dp = DetectPlan(2, sizes, STRIDES, 'cuda', num_classes=80, ld_cls=84, head=HeadOptions(norm_on_bbox=False, centerness_on_reg=False))
    dp.bind(flat.cuda(), rc.cuda(), torch.ones(5, device='cuda'))
    shp = tuple(int(v) for v in d['img_shape'])
    dp.set_meta([shp] * 2, [d['scale_factor']] * 2, True)
    dp.run()
    torch.cuda.synchronize()
    ref = [(T(d[f'det{i}']), T(d[f'lab{i}'])) for i in range(2)]
    assert all(len(r[0]) > 0 for r in ref)
    _match(dp.dets, dp.labels, dp.count, ref, 2)


def test_simple_test_plain_model_vs_reference(golden):
    """simple_test (bf16 forward + detect) of the plain model: the reference's confident detections are found with near-identical
    boxes (test_simple_test_vs_oracle's criteria)."""
    d = golden('sweep_tiny_plain.npz')
    sd = HR.plain_state_dict(0)
    sd['bbox_head.conv_cls.bias'] = torch.full((80,), float(d['cls_bias']))
    sd['bbox_head.conv_reg.bias'] = sd['bbox_head.conv_reg.bias'] + float(d['reg_bias_add'])
    model = build_plain()
    model.load_state_dict(sd)
    shp = tuple(int(v) for v in d['img_shape'])
    metas = [dict(img_shape=shp, scale_factor=d['scale_factor'])] * 2
    res = model.simple_test(T(d['img']).cuda(), metas, rescale=True)
    assert len(res) == 2 and all(len(r) == 80 for r in res)
    for i in range(2):
        rb, rl = d[f'det{i}'], d[f'lab{i}']
        got = np.concatenate(res[i])
        assert abs(len(got) - len(rb)) <= max(2, len(rb) // 10)
        found = 0
        top = np.argsort(-rb[:, 4])[:20]
        for j in top:
            cand = res[i][int(rl[j])]
            if len(cand):
                dist = np.abs(cand[:, :4] - rb[j, :4]).max(1)
                k = dist.argmin()
                found += int(dist[k] < 1.0 and abs(cand[k, 4] - rb[j, 4]) < 0.02)
        assert found >= len(top) - 2, found          # (score ties at the 100-detection cut may swap the last entries)


def test_plain_train_step_vs_reference_and_restatement(golden):
    """The checks of test_step_gpu.test_train_step_vs_reference_and_oracle on the plain head (net_tiny_plain.npz): against the
    reference's fp32 values, against the bf16-emulating restatement, gradients by e_hip <= 1.6 e_emu + 5e-3 against the fp32
    restatement; assignment identical; a second step gives the same bits.  exp() amplifies bf16 noise in loss_bbox: where the emulating
    restatement itself misses the 3e-2 bar against fp32, HIP is held to 1.6 x its error + 5e-3 instead (the gradient rule)."""
    d = golden('net_tiny_plain.npz')
    B = int(d['B'])
    model = build_plain()
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
    sd = HR.plain_state_dict(0)
    with oracle_threads():
        lem, gem, aux = HR.train_step(sd, img, gtb, gtl, None, opts=HR.PLAIN, emulate_bf16=True)
        l32, g32, aux32 = HR.train_step(sd, img, gtb, gtl, None, opts=HR.PLAIN, emulate_bf16=False)
    for k in got:
        e_emu = abs(lem[k] - float(d[k])) / abs(float(d[k]))
        e_hip = abs(got[k] - float(d[k])) / abs(float(d[k]))
        print(k, 'hip', got[k], 'emu-bf16', lem[k], 'restatement-fp32', l32[k], 'reference-fp32', float(d[k]), 'e_hip', e_hip, 'e_emu', e_emu)
        assert e_hip <= (3e-2 if e_emu <= 3e-2 else 1.6 * e_emu + 5e-3), (k, e_hip, e_emu)
        assert got[k] == pytest.approx(lem[k], rel=3e-3), (k, got[k], lem[k])
    plan = next(iter(model._engine.plans.values()))
    st = model.store
    assert st.ctr_on_cls and plan.bufs['cls_logits'].shape[1] == 84
    logits = plan.bufs['cls_logits'].cpu()
    ref_cls, ref_ctr = levels_to_flat([c.detach() for c in aux['cls']]), levels_to_flat([c.detach() for c in aux['ctr']])
    assert rel_l2(logits[:, :80], ref_cls) < 5e-3
    # the centerness logit is one more row of the same launch on the same activations, its weights drawn like conv_cls's: the same
    # ABSOLUTE noise as a class logit (relative to its own size - no focal-prior bias of -4.6 in it - that is percents)
    rms = lambda t: float(t.double().pow(2).mean().sqrt())
    e_cls, e_ctr = rms(logits[:, :80] - ref_cls), rms(logits[:, 80:81] - ref_ctr)
    print('logit rms error: classes', e_cls, 'centerness', e_ctr)
    assert e_ctr <= 2.0 * e_cls
    assert float(logits[:, 81:].abs().max()) == 0.0
    _, raux = HR.fcos_loss(aux32['cls'], aux32['reg'], aux32['ctr'], gtb, gtl, None, opts=HR.PLAIN, return_aux=True)
    assert torch.equal(plan.lossplan.labels.cpu(), raux['labels'])
    assert torch.equal(plan.lossplan.assign_idx.cpu().long(), raux['assign_idx'])
    named = dict(model.named_parameters())
    keys = [str(k) for k in d['grad_keys']]
    assert sorted(keys) == sorted(k for k, p in named.items() if p.requires_grad)
    bad = []
    for k in keys:
        e_hip, e_emu = rel_l2(named[k].grad.cpu(), g32[k]), rel_l2(gem[k], g32[k])
        if float(g32[k].norm()) > 0 and e_hip > 1.6 * e_emu + 5e-3:
            bad.append((k, e_hip, e_emu))
    assert not bad, bad[:10]
    ref_norms = dict(zip(keys, d['grad_norms']))
    nerr = {k: abs(float(named[k].grad.norm()) - ref_norms[k]) / (ref_norms[k] + 1e-12) for k in keys}
    print('worst grad-norm err vs fp32 reference:', sorted(nerr.items(), key=lambda kv: -kv[1])[:5])
    assert max(nerr.values()) < 0.2
    # rows that no parameter owns stay without gradient: classes .. centerness row, behind it, and conv_reg's fifth row onwards
    assert float(st.tview('head.cls_w', st.grad)[81:].abs().max()) == 0.0 and float(st.tview('head.regctr_w', st.grad)[4:].abs().max()) == 0.0
    got2, grad2 = step()
    assert got2 == got and torch.equal(grad2, grad)


def test_flat_sgd_with_grad_clip_on_the_bias_free_head(golden):
    """One FlatSGD step with grad_clip max_norm=35 (configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_coco.py): the clipping norm is the
    host norm over the reference's parameter set, there is no tower bias region to update or count, padding rows stay zero."""
    from dsl_amd.optim import FlatSGD
    d = golden('net_tiny_plain.npz')
    B = int(d['B'])
    model = build_plain()
    st = model.store
    opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.),
                  grad_clip=dict(max_norm=35, norm_type=2))
    img = T(d['img'])
    gtb, gtl = [T(d[f'gt{i}']) for i in range(B)], [T(d[f'gl{i}']) for i in range(B)]
    losses = model.forward_train(img.cuda(), [dict()] * B, gtb, gtl)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    keys = [k for k, p in named.items() if p.requires_grad]
    assert not [k for k in keys if HR.is_tower_bias(k)] and sorted(keys) == sorted(str(k) for k in d['grad_keys'])
    host = float(torch.sqrt(sum((named[k].grad.double() ** 2).sum() for k in keys)))
    assert float(st.grad.double().norm()) == pytest.approx(host, rel=1e-6)        # nothing outside the reference's parameters
    before = st.train.clone()
    gn = opt.gnorm_sq
    opt.step()
    torch.cuda.synchronize()
    gsq = opt.gnorm_sq if opt.gnorm_sq is not None else gn
    assert float(gsq.sqrt()) == pytest.approx(host, rel=1e-4)
    assert not [k for k in st.train_regions if 'bbox_head' in k and k.endswith('.conv.bias')]
    assert int(st.group.sum()) == sum(n for k, (o_, n, s_) in st.train_regions.items() if k.endswith('.conv.bias') or k in ('head.cls_b', 'head.regctr_b'))
    assert not torch.equal(before, st.train) and torch.isfinite(st.train).all()
    assert float(st.tview('head.cls_w')[81:].abs().max()) == 0.0 and float(st.tview('head.cls_w')[80].abs().max()) > 0.0
    assert float(st.tview('head.regctr_w')[4:].abs().max()) == 0.0 and float(st.tview('head.cls_b')[81:].abs().max()) == 0.0
    assert float(st.tview('head.regctr_b')[4:].abs().max()) == 0.0


def test_plain_head_on_rla_backbone_step_vs_restatement():
    """The plain head under RLA_ResNet (engine_rla builds the backbone's lists, the head's are engine.py's: the centerness row in
    the classification predictor, bias-free towers, the RLA segment order and its buckets) at 128 x 192: the checks of
    test_plain_train_step_vs_reference_and_restatement with tests/head_options_ref.py composed with the oracle's RLA forward -
    fp32 values (no reference fixture of this combination exists: the fp32 restatement stands in), the bf16-emulating restatement,
    gradients by e_hip <= 1.6 e_emu + 5e-3 (test_rla_gpu's noise-floor rule for parameters whose emulation is itself > 25 % off),
    identical assignment, and a second step with the same bits."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from oracle import fcos_oracle as O
    from oracle import rla_oracle as RO
    from test_rla_gpu import rla_model_cfg
    sd = HR.plain_state_dict(0, backbone='rla')
    model = build_detector(rla_model_cfg(**PLAIN_HEAD))
    assert set(model.state_dict()) == set(sd) and len(sd) == 465 - 8
    model.load_state_dict(sd)
    model = model.cuda()
    rng = np.random.RandomState(1)
    g = torch.Generator().manual_seed(3)
    H, W, B = 128, 192, 2
    img = (torch.randn(B, 3, H, W, generator=g) * 40).bfloat16().float()
    gtb = [T(O.synth_boxes(rng, 4, H=H, W=W, lo=8, hi=min(H, W))) for _ in range(B)]
    gtl = [T(rng.randint(0, 80, len(b)).astype('int64')) for b in gtb]

    def step():
        model.store.grad.zero_()
        losses = model.forward_train(img.cuda(), [dict()] * B, gtb, gtl)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        return {k: float(v.detach()) for k, v in losses.items()}, model.store.grad.clone()
    got, grad = step()
    with oracle_threads():
        l32, g32, aux32 = HR.train_step(sd, img, gtb, gtl, None, opts=HR.PLAIN, emulate_bf16=False, backbone='rla')
        lem, gem, _ = HR.train_step(sd, img, gtb, gtl, None, opts=HR.PLAIN, emulate_bf16=True, backbone='rla')
    for k in got:
        e_emu, e_hip = abs(lem[k] - l32[k]) / abs(l32[k]), abs(got[k] - l32[k]) / abs(l32[k])
        print(k, 'hip', got[k], 'emu-bf16', lem[k], 'fp32', l32[k], 'e_hip', e_hip, 'e_emu', e_emu)
        assert e_hip <= (3e-2 if e_emu <= 3e-2 else 1.6 * e_emu + 5e-3), (k, e_hip, e_emu)
        assert got[k] == pytest.approx(lem[k], rel=3e-3), (k, got[k], lem[k])
    plan = next(iter(model._engine.plans.values()))
    _, raux = HR.fcos_loss([t.detach() for t in aux32['cls']], [t.detach() for t in aux32['reg']], [t.detach() for t in aux32['ctr']],
                           gtb, gtl, None, opts=HR.PLAIN, return_aux=True)
    assert torch.equal(plan.lossplan.labels.cpu(), raux['labels'])
    assert torch.equal(plan.lossplan.assign_idx.cpu().long(), raux['assign_idx'])
    named = dict(model.named_parameters())
    tk = RO.trainable_keys(sd)
    assert sorted(k for k, p in named.items() if p.requires_grad) == sorted(tk)
    bad, noisy = [], []
    for k in tk:
        e_hip, e_emu = rel_l2(named[k].grad.detach().cpu(), g32[k]), rel_l2(gem[k], g32[k])
        if e_emu > 0.25:
            noisy.append(k)
            continue
        if float(g32[k].norm()) > 0 and e_hip > 1.6 * e_emu + 5e-3:
            bad.append((k, e_hip, e_emu))
    print(len(noisy), 'parameters below the noise floor')
    assert not bad, bad[:10]
    assert len(noisy) <= 60, noisy          # (test_rla_gpu.test_rla_train_step_vs_oracle's count)
    assert not [k for k in noisy if k.startswith('bbox_head.')]
    st = model.store
    assert float(st.tview('head.cls_w', st.grad)[81:].abs().max()) == 0.0 and float(st.tview('head.cls_w', st.grad)[80].abs().max()) > 0.0
    assert float(st.tview('head.regctr_w', st.grad)[4:].abs().max()) == 0.0
    got2, grad2 = step()
    assert got2 == got and torch.equal(grad2, grad)


def test_plain_config_trains_through_train_detector(tmp_path):
    """configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_coco.py's model, optimizer, grad_clip, lr and runner sections (restated: the GPU box
    has no reference tree; tests/test_head_options_cpu.py builds the real file) through train_detector on synthetic batches: two
    epochs of three iterations with checkpoints, bbox evaluation and a resume - finite losses,
    the constant warm-up's learning rate, no tower bias anywhere, padding rows zero, the centerness row trained."""
    import json
    import os
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.apis import train_detector
    from dsl_amd.data import SyntheticValLoader, synth_boxes
    from dsl_amd.registry import Config, build_detector
    H, W, n_it = 128, 192, 3
    rng = np.random.RandomState(4)
    g = torch.Generator().manual_seed(4)
    batches = []
    for _ in range(n_it):
        img = (torch.randn(2, 3, H, W, generator=g) * 30).bfloat16().float().cuda()
        gtb = [T(synth_boxes(rng, 4, H=H, W=W, lo=12, hi=120)) for _ in range(2)]
        gtl = [T(rng.randint(0, 80, len(b)).astype('int64')) for b in gtb]
        metas = [dict(filename=f'im{i}.jpg', ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3),
                      scale_factor=np.ones(4, np.float32), flip=False) for i in range(2)]
        batches.append(dict(img=img, img_metas=metas, gt_bboxes=gtb, gt_labels=gtl))

    class Loader:
        CLASSES = tuple(f'class_{i}' for i in range(80))

        def __len__(self):
            return n_it

        def __iter__(self):
            return iter(batches)

    def config(epochs, resume=None):
        cfg = Config(dict(
            model=fcos_model_cfg(**PLAIN_HEAD), data=dict(samples_per_gpu=2, workers_per_gpu=2),
            optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001, paramwise_cfg=dict(bias_lr_mult=2., bias_decay_mult=0.)),
            optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
            lr_config=dict(policy='step', warmup='constant', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11]),
            runner=dict(type='EpochBasedRunner', max_epochs=epochs), checkpoint_config=dict(interval=1),
            log_config=dict(interval=1, hooks=[dict(type='TextLoggerHook')]), custom_hooks=[dict(type='NumClassCheckHook')],
            log_level='WARNING', load_from=None, resume_from=resume, workflow=[('train', 1)], work_dir=str(tmp_path)))
        cfg.val_dataloader = SyntheticValLoader(n_images=2, num_classes=80, H=H, W=W)
        cfg.evaluation = dict(interval=1, metric='bbox')
        return cfg
    import warnings
    model = build_detector(config(2).model)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model.init_weights()
    runner = train_detector(model, [Loader()], config(2), distributed=False, validate=True)
    torch.cuda.synchronize()
    det = runner._det(runner.model)
    st = det.store
    assert runner.iter == 2 * n_it and runner.epoch == 2 and runner.optimizer.max_norm == 35.0
    assert [round(g_['lr'], 9) for g_ in runner.optimizer.param_groups][:2] == [round(0.01 / 3, 9), round(0.02 / 3, 9)]
    assert torch.isfinite(st.train).all()
    recs = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'train.log.json'))]
    recs = [r for r in recs if 'loss_cls' in r]
    assert len(recs) == 2 * n_it and all(np.isfinite(v) for r in recs for k, v in r.items() if k.startswith('loss'))
    print('loss per iteration:', [round(r['loss'], 4) for r in recs])
    assert not [k for k in det.state_dict() if HR.is_tower_bias(k)]
    assert float(st.tview('head.cls_w')[81:].abs().max()) == 0.0 and float(st.tview('head.regctr_w')[4:].abs().max()) == 0.0
    ck = torch.load(os.path.join(str(tmp_path), 'latest.pth'), map_location='cpu')
    assert set(ck['state_dict']) == set(HR.plain_state_dict(0)) and torch.equal(ck['state_dict']['bbox_head.conv_centerness.weight'],
                                                                               det.state_dict()['bbox_head.conv_centerness.weight'].cpu())
    # the centerness row was trained (its initial values are the store's seeded draw)
    fresh = build_detector(config(2).model)
    assert not torch.equal(fresh.state_dict()['bbox_head.conv_centerness.weight'], ck['state_dict']['bbox_head.conv_centerness.weight'])
    # resume for a third epoch into a new model: weights and momentum come from the checkpoint
    again = build_detector(config(3).model)
    r2 = train_detector(again, [Loader()], config(3, resume=os.path.join(str(tmp_path), 'latest.pth')), distributed=False, validate=False)
    torch.cuda.synchronize()
    assert r2.iter == 3 * n_it and r2.epoch == 3 and torch.isfinite(r2._det(r2.model).store.train).all()
