"""The head kernels on the generated cases of tests/head_cases.py (test_head_cases_cpu.py shows what each case reaches and that every
mixture fit's decisions lie 1e-9 from their thresholds): dsl_atss_assign and dsl_paa_assign bit for bit against atss_ref / paa_ref,
dsl_paa_reassign on written candidates and on the models' candidate losses, the four heads' losses and gradients against float64
autograd with the bars of the heads' own check_loss functions, and a reused plan whose next batch has fewer boxes."""
import ctypes as C_

import pytest
import torch

import atss_ref as AR
import head_cases as HC
import paa_ref as PR
import test_atss_gpu as TA
import test_gfl_gpu as TG
import test_ld_gpu as TL
import test_paa_gpu as TP

pytestmark = pytest.mark.gpu


def nbox(c):
    return sum(len(g) for g in c['gts'])


def max_gt(c):
    return nbox(c) if c['name'] == 'GT' else 64          # GT: a box count equal to max_gt


def entry(plan, name):
    from dsl_amd import _lib as L
    L.check(getattr(L.lib, name)(C_.byref(plan.paa), L.stream_ptr()), name)


# ---- first assignments ----------------------------------------------------------------------------------------------------------
def atss_state(plan):
    return [t.cpu().clone() for t in (plan.labels, plan.assign_idx, plan.cls_weight, plan.bbox_targets, plan.npos, plan.stats, plan.pos_weight)]


@pytest.mark.parametrize('name', ['G70', 'G2L', 'GT', 'R'])
def test_atss_assign_bit_exact_vs_model(name):
    c, a = HC.case(name), HC.ref(name)['atss']
    plan = TA.assigned_plan(c, max_gt(c))
    torch.cuda.synchronize()
    got = atss_state(plan)
    assert torch.equal(got[0], a['labels']) and torch.equal(got[1], a['assign_idx'])
    assert torch.equal(got[2], a['cls_weight']) and torch.equal(got[3], a['targets'])
    assert got[4].tolist() == a['npos'] and float(got[5][0]) == float(a['num_total']) and float(got[5][2:].abs().max()) == 0.0
    pos = (a['labels'] < c['C']).nonzero().view(-1)
    anchors = AR.flat_anchors(c['sizes'], c['B'], c['anchor_scale'], c['strides']).double()
    csum = float(AR.centerness_target(anchors[pos], a['targets'].double()[pos]).sum())
    print(name, 'positives', a['npos'], 'centerness sum', float(got[5][1]), csum)
    assert len(pos) > 0 and float(got[5][1]) == pytest.approx(csum, rel=1e-5)          # test_atss_gpu's tolerance for stats[1]
    assert bool((got[6] == 1).all())
    again = TA.assigned_plan(c, max_gt(c))
    plan.assign()
    torch.cuda.synchronize()
    for p in (again, plan):
        assert all(torch.equal(u, v) for u, v in zip(got, atss_state(p)))


@pytest.mark.parametrize('name', HC.ASSIGN_CASES)
def test_paa_assign_bit_exact_vs_model(name):
    c, p = HC.case(name), HC.ref(name)['paa']
    plan = TP.assigned_plan(c, max_gt(c))
    torch.cuda.synchronize()
    got = TP.state(plan)
    assert torch.equal(got[1], p['cand_gt']) and torch.equal(got[2], got[1]) and torch.equal(got[0], p['labels'])
    assert torch.equal(got[3], p['cls_weight']) and torch.equal(got[4], p['targets'])
    assert bool((got[5] == 1).all()) and got[6].tolist() == [0] * c['B'] and float(got[7].abs().max()) == 0.0
    print(name, 'candidates', int((got[1] >= 0).sum()), 'of', c['M'])
    again = TP.assigned_plan(c, max_gt(c))
    plan.assign()
    torch.cuda.synchronize()
    for q in (again, plan):
        assert all(torch.equal(u, v) for u, v in zip(got[:8], TP.state(q)[:8]))


# ---- the reassignment -----------------------------------------------------------------------------------------------------------
def check_reassign(c, plan, cand, re, want_iou, exact_iou=False):
    """test_paa_gpu.test_reassign_on_the_fixture_losses's comparison against a paa_ref.reassign result: integers exact, the IoU
    targets to rtol 1e-5 / atol 1e-6 (exact_iou: the written values, kept or cleared), their sum to rel 1e-5."""
    got = TP.state(plan)
    nb, kept = len(re['boxes']), re['kept']
    for k, b in enumerate(re['boxes']):
        print(c['name'], 'box', k, 'samples', len(b['index']), 'iterations', b['n_iter'], 'flag', b['flag'], 'kept', b['npos'],
              'device', int(got[10][k]), int(got[11][k]))
    assert got[10][:nb].tolist() == [b['n_iter'] for b in re['boxes']] and got[11][:nb].tolist() == [b['flag'] for b in re['boxes']]
    if nb < len(got[10]):
        assert float(got[10][nb:].abs().max()) == 0 and float(got[11][nb:].abs().max()) == 0
    assert torch.equal(got[0], re['labels']) and got[6].tolist() == re['npos']
    minus = torch.full_like(cand, -1)
    assert torch.equal(got[1], cand) and torch.equal(got[2], torch.where(kept, cand, minus))
    assert torch.equal(got[5], (kept | (cand < 0)).float())          # box weight 0 where demoted
    want = want_iou.double() * kept.double()
    print(c['name'], 'iou_target: largest deviation', float((got[9].double() - want).abs().max()), 'sum', float(got[7][1]), float(want.sum()))
    assert torch.allclose(got[9].double(), want, rtol=1e-5, atol=1e-6)
    if exact_iou:
        assert torch.equal(got[9], want_iou * kept.float())
    assert float(got[7][0]) == float(sum(re['npos'])) and float(got[7][1]) == pytest.approx(float(want.sum()), rel=1e-5, abs=1e-6)
    assert float(got[7][2:].abs().max()) == 0.0
    return got


def test_reassign_on_written_candidates():
    """Sample counts 80, 70, 65, 64, 63, 2, 1 and 0, levels cut at topk and levels short of it, bit-equal losses, both flag-2 kinds,
    an image without boxes between two that have some.  The reassignment reads nothing it wrote: a second launch gives the same."""
    m = HC.mix()
    plan = TP.assigned_plan(m)
    for dst, src in ((plan.cand_gt, m['cand_gt']), (plan.assign_idx, m['cand_gt']), (plan.labels, m['labels0']), (plan.pos_loss, m['pos_loss']),
                     (plan.iou_target, m['iou_target'])):
        dst.copy_(src)
    entry(plan, 'dsl_paa_reassign')
    torch.cuda.synchronize()
    got = check_reassign(m, plan, m['cand_gt'], m['re'], m['iou_target'], exact_iou=True)
    assert sorted(set(got[11][:len(m['re']['boxes'])].tolist())) == [0, 1, 2]
    entry(plan, 'dsl_paa_reassign')
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(got, TP.state(plan)))


def model_iou(c, asg, re):
    return PR.iou_targets(c['reg'], c['scales'], asg, re, c['sizes'], c['B'], c['anchor_scale'], c['stds'], c['strides'])


@pytest.mark.parametrize('name', ['G70', 'G64'])
def test_pos_loss_and_reassign_on_the_models_losses(name):
    """dsl_paa_pos_loss against paa_ref.pos_loss (test_paa_gpu.test_pos_loss_vs_reference's bar, rel 1e-5), then the reassignment fed
    paa_ref.pos_loss(...).float(): 70 samples (G70) and exactly 64 (G64) for the big box."""
    c, r = HC.case(name), HC.ref(name)
    plan = TP.refined_plan(c, dict(pos_loss=r['pl32'].numpy()))
    got, want = plan.own_pos_loss.cpu().double(), r['pos_loss']
    cand = r['paa']['cand_gt'] >= 0
    rel = ((got - want).abs() / want.clamp(min=1e-12))[cand]
    print(name, 'pos_loss: largest relative deviation', float(rel.max()), 'over', int(cand.sum()), 'candidates')
    assert float(rel.max()) <= 1e-5 and float(got[~cand].abs().max()) == 0.0 and int(cand.sum()) > 50
    st = check_reassign(c, plan, r['paa']['cand_gt'], r['re'], model_iou(c, r['paa'], r['re']))
    assert len(r['re']['boxes'][0]['index']) == (70 if name == 'G70' else 64) and sum(r['re']['npos']) > 0
    entry(plan, 'dsl_paa_reassign')
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(st, TP.state(plan)))


def test_whole_chain_on_the_devices_own_losses():
    """assign -> pos_loss -> reassign on G70 with no array fed: paa_ref.reassign of the losses read back, whose margins come first."""
    c, r = HC.case('G70'), HC.ref('G70')
    plan = TP.refined_plan(c, None, feed=False)
    own = plan.pos_loss.cpu()
    assert torch.equal(own, plan.own_pos_loss.cpu())
    re = HC.reassign(c, r['paa'], own.numpy())
    thin = HC.thin_margins(re)
    print('margins of the read-back losses', [HC.box_margins(b) for b in re['boxes']])
    assert not thin, f'the device\'s own losses put a mixture fit within {HC.MARGIN} of a threshold (box, flag, margin, gap): {thin}'
    check_reassign(c, plan, r['paa']['cand_gt'], re, model_iou(c, r['paa'], re))
    assert [len(b['index']) for b in re['boxes']] == [len(b['index']) for b in r['re']['boxes']]


# ---- losses and gradients -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['G70', 'G2L'])
@pytest.mark.parametrize('head', ['atss', 'gfl', 'ld', 'paa'])
def test_loss_and_gradients_vs_float64(head, name):
    """The heads' own check_loss functions and bars (losses rel 1e-4, bf16 gradients 2^-8, padding columns zero) on G70 - five
    classes, twenty workgroups, an image without a box - and on the two-level G2L; GFL and LD with reg_max 7."""
    c = HC.case(name)
    if head == 'atss':
        plan = TA.check_loss(c, c['cls'], c['reg'], c['ctr'], c['scales'])[0]
    elif head == 'gfl':
        plan = TG.check_loss(c, c['cls'], c['dist'], c['scales'])[0]
        assert (plan.LD_RC, plan.LD_GRC) == (32, 64)
    elif head == 'ld':
        plan = TL.check_loss(c, c['cls'], c['dist'], c['scales'], c['soft'], c['soft_scales'])[0]
        assert float(plan.losses[3].cpu()) > 0
    else:
        d = dict(pos_loss=HC.ref(name)['pl32'].numpy())
        plan = TP.refined_plan(c, d)
        plan.loss()
        torch.cuda.synchronize()
        re = TP.check_loss(c, d, plan)
        assert sum(re['npos']) > 0
    nl = len(c['sizes'])
    assert (nl == len(plan.g_scales) or float(plan.g_scales[nl:].abs().max()) == 0.0) and bool(torch.isfinite(plan.losses).all())
    if name == 'G70':          # the image without a box has no positive
        assert plan.npos.tolist()[1] == 0 and min(plan.npos.tolist()[0], plan.npos.tolist()[2]) > 0


# ---- a reused plan ---------------------------------------------------------------------------------------------------------------
def full_state(plan, head):
    base = TP.state(plan) if head == 'paa' else atss_state(plan)
    return base + [t.cpu().clone() for t in (plan.losses, plan.g_cls, plan.g_rc, plan.g_scales, plan.logvec)]


def run_batch(plan, c, head):
    plan.set_targets(c['gts'], c['gls'], None, c['pads'])
    plan.assign()
    if head == 'paa':
        plan.refine()
    plan.loss()
    torch.cuda.synchronize()
    return full_state(plan, head)


def bound_plan(c, head):
    if head == 'paa':
        return TP.assigned_plan(c, nbox(HC.case('GT')))
    plan = TA.assigned_plan(c, nbox(HC.case('GT')))
    cl = torch.full((plan.M, plan.LD_CLS), float('nan'))
    cl[:, :c['C']] = c['cls']
    rc = torch.full((plan.M, 8), float('nan'))
    rc[:, :4], rc[:, 4] = c['reg'], c['ctr']
    plan.bind_outputs(cl.cuda(), rc.cuda(), c['scales'].cuda())
    plan._keep = (cl, rc)
    return plan


@pytest.mark.parametrize('head', ['atss', 'paa'])
def test_reused_plan_with_fewer_boxes_equals_a_fresh_one(head):
    """One plan with max_gt = GT's 13 boxes runs GT, then a batch with one box, then one without any: every output of the second run
    is a fresh plan's - per-box arrays, per-image counts and the sums of the block records included -, the third is all background."""
    c = HC.case('GT')
    none, nol = torch.zeros(0, 4), torch.zeros(0, dtype=torch.long)
    one = dict(c, gts=[none, none, c['gts'][0][:1], none], gls=[nol, nol, c['gls'][0][:1], nol])
    empty = dict(c, gts=[none] * 4, gls=[nol] * 4)
    plan = bound_plan(c, head)
    first = run_batch(plan, c, head)
    second = run_batch(plan, one, head)
    fresh = run_batch(bound_plan(one, head), one, head)
    assert all(torch.equal(u, v) for u, v in zip(second, fresh))
    assert not all(torch.equal(u, v) for u, v in zip(first, second))
    if head == 'paa':
        assert int(first[10].max()) > 0 and second[10][1:].tolist() == [0] * (nbox(c) - 1) and second[11][1:].tolist() == [0] * (nbox(c) - 1)
        assert sum(second[6].tolist()) > 0
    else:
        assert second[4].tolist()[2] > 0 and second[4].tolist()[:2] == [0, 0]
    third = run_batch(plan, empty, head)
    assert bool((third[0] == c['C']).all()) and bool((plan.assign_idx.cpu() == -1).all()) and plan.npos.tolist() == [0] * 4
    assert float(plan.bbox_targets.abs().max()) == 0.0
    losses = plan.losses.cpu()
    assert float(losses[1]) == 0.0 and float(losses[2]) == 0.0 and float(losses[0]) > 0 and bool(torch.isfinite(losses).all())
    assert float(plan.g_rc.float().abs().max()) == 0.0 and bool(torch.isfinite(plan.g_cls.float()).all())
    st = plan.stats.cpu()
    if head == 'paa':
        assert float(st.abs().max()) == 0.0 and float(third[10].abs().max()) == 0 and float(third[11].abs().max()) == 0
        assert bool((third[1] == -1).all()) and float(third[9].abs().max()) == 0.0
    else:
        assert float(st[0]) == 4.0 and float(st[1:].abs().max()) == 0.0          # sum_i max(0, 1)
    assert all(torch.equal(u, v) for u, v in zip(third, run_batch(bound_plan(empty, head), empty, head)))
