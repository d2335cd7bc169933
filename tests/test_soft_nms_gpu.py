"""The Soft-NMS pass of detect.hip (dsl_det_desc.nms_method) through the C ABI, against tests/soft_nms_ref.py: labels, boxes and
order identical to the model, rescored scores within soft_nms_ref.score_rtol.  tests/test_soft_nms_cpu.py proves that no two
scores that compete in these inputs are closer than 100 x that tolerance, so nothing here is compared 'up to ties'.

The issue's shapes - one or two levels of 4 x 6 and 2 x 3 locations - hold at most 30 candidates per class, short of the wave size;
levels='long' (8 x 12 + 2 x 3 locations, a cluster of 70) adds the list that more than one wave runs."""
import numpy as np
import pytest
import torch

import aug_ref as A
import detect_ref as R
import soft_nms_ref as S
from util import levels_to_flat

pytestmark = pytest.mark.gpu
PAD = 50.0


def sizes_of(case):
    return [tuple(c.shape[2:]) for c in case.cls]


def make_plan(case, method, sigma=0.5, min_score=1e-3, **kw):
    from dsl_amd.sweep import DetectPlan
    ld = (case.C + 4) // 4 * 4
    sizes = sizes_of(case)
    return DetectPlan(case.n, sizes, A.STRIDES[:len(sizes)], 'cuda', num_classes=case.C, nms_pre=case.nms_pre, max_per_img=case.max_per_img,
                      score_thr=case.score_thr, iou_thr=case.iou_thr, ld_cls=ld, nms_method=S.METHODS.get(method, 0), soft_sigma=sigma,
                      soft_min_score=min_score, **kw)


def bind(dp, case):
    f = levels_to_flat(case.cls)
    cls = torch.full((f.shape[0], dp.desc.ld_cls), PAD)
    cls[:, :case.C] = f
    rc = torch.zeros(f.shape[0], 8)
    rc[:, :4] = levels_to_flat(case.raw)
    rc[:, 4] = levels_to_flat(case.ctr)[:, 0]
    dp.bind(cls.cuda(), rc.cuda(), torch.ones(5, device='cuda'))
    dp.set_meta(case.img_shapes, case.scale_factors, case.rescale)


def run(case, method, **kw):
    dp = make_plan(case, method, **kw)
    bind(dp, case)
    dp.run()
    torch.cuda.synchronize()
    out = []
    for i in range(case.n):
        k = int(dp.count[i])
        assert 0 <= k <= case.max_per_img
        assert float(dp.dets[i, k:].abs().sum()) == 0
        out.append((dp.dets[i, :k].cpu(), dp.labels[i, :k].cpu()))
    return out


def same(got, ref, rtol, what=''):
    (gb, gl), (rb, rl) = got, ref[:2]
    print(what, 'kept', len(gb), 'model', len(rb))
    assert len(gb) == len(rb), (len(gb), len(rb))
    if len(gb) == 0:
        return
    rel = ((gb[:, 4].double() - rb[:, 4].double()).abs() / rb[:, 4].double()).max()
    print(what, 'max rel |score - model|', float(rel), 'allowed', rtol, 'max |box - model|', float((gb[:, :4] - rb[:, :4]).abs().max()))
    assert torch.equal(gl, rl)
    assert torch.equal(gb[:, :4], rb[:, :4].float())
    assert float(rel) <= rtol


@pytest.mark.parametrize('min_score', [S.LONG_MIN_SCORE, 1e-3])
@pytest.mark.parametrize('method', ['linear', 'naive', 'gaussian'])
@pytest.mark.parametrize('levels,C,max_per_img', [(1, 3, 100), (2, 80, 100), (2, 3, 5), (1, 80, 5), ('long', 3, 100), ('long', 80, 5)])
def test_matches_the_model(levels, C, max_per_img, method, min_score):
    """min_score 1e-30 keeps the whole cluster in the running (29 decays of its last pick; 'long': a list of 70), 1e-3 lets its tail
    disappear.  max_per_img = 5 is smaller than the cluster's picks: the kernel stops the class there, the model runs it to its end."""
    case = S.case(levels, C, max_per_img)
    # every pick of a class decays each remaining candidate of the class at most once, and the largest class is the cluster
    n_decays = S.cluster_size(levels) - 1
    for i, (g, r) in enumerate(zip(run(case, method, min_score=min_score), S.detect(case, method, min_score=min_score, bound=False))):
        same(g, r, S.score_rtol(n_decays, method), f'image {i}')


@pytest.mark.parametrize('method', ['linear', 'naive', 'gaussian'])
def test_no_candidates(method):
    case = S.exact_case('empty')
    assert all(len(b) == 0 for b, _ in run(case, method))


@pytest.mark.parametrize('method', ['linear', 'naive', 'gaussian'])
def test_min_score_above_every_decayed_score(method):
    """One candidate of the cluster at score 1.0f, 23 at 0.5f (exact sigmoids): each of them is at most 0.5 * (1 - 0.55) < 0.45 after
    the first pick and is dropped.  No emitted score went through a decay: n_decays = 0, the scores are the model's bits."""
    case = S.exact_case('drop')
    n_decays = 0
    for g, r in zip(run(case, method, min_score=0.45), S.detect(case, method, min_score=0.45)):
        assert len(r[0]) == 1 and r[2]['n_decays'] == n_decays
        same(g, r, S.score_rtol(n_decays, method))


@pytest.mark.parametrize('C', [3, 80])
def test_method_0_with_zeroed_fields_keeps_the_bits_of_a_descriptor_built_the_old_way(C):
    """nms_method = 0, soft_sigma = soft_min_score = 0: the hard NMS, bit for bit what a DetectPlan that never sets the fields gives,
    with the workspace size of before."""
    from dsl_amd.sweep import DetectPlan
    case = S.case(2, C, 100, iou_thr=0.6)
    new = make_plan(case, None, sigma=0.0, min_score=0.0)
    sizes = sizes_of(case)
    old = DetectPlan(case.n, sizes, A.STRIDES[:len(sizes)], 'cuda', num_classes=case.C, nms_pre=case.nms_pre, max_per_img=case.max_per_img,
                     score_thr=case.score_thr, iou_thr=case.iou_thr, ld_cls=new.desc.ld_cls)
    assert new.desc.workspace_bytes == old.desc.workspace_bytes
    soft = make_plan(case, 'linear')
    assert soft.desc.workspace_bytes == old.desc.workspace_bytes + case.n * R.CAND_CAP * 4
    outs = []
    for dp in (new, old):
        bind(dp, case)
        dp.run()
        torch.cuda.synchronize()
        outs.append((dp.dets.cpu(), dp.labels.cpu(), dp.count.cpu()))
    assert int(outs[0][2].min()) >= 2
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    for i, r in enumerate(R.detect(case)):
        k = int(outs[0][2][i])
        assert k == len(r[0]) and torch.equal(outs[0][1][i, :k], r[1])


def test_bad_fields_are_refused():
    case = S.exact_case('empty')
    for kw, msg in ((dict(sigma=0.0), 'soft_sigma must be > 0'), (dict(min_score=-1.0), 'soft_min_score must be >= 0')):
        dp = make_plan(case, 'gaussian', **kw)
        bind(dp, case)
        with pytest.raises(RuntimeError, match=msg):
            dp.run()
    dp = make_plan(case, 'linear')
    dp.desc.nms_method = 4
    bind(dp, case)
    with pytest.raises(RuntimeError, match='nms_method must be a DSL_NMS_'):
        dp.run()


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_aug_finish_runs_one_soft_nms_over_the_pooled_views(method):
    """Two views of a 64 x 96 image - itself and its half-size horizontal flip -, Soft-NMS in finish, against the model on
    aug_ref.collect's pooled candidates; the cluster's 14 + 11 candidates meet in one class."""
    from dsl_amd.sweep import AugMerge, DetectPlan
    views, metas = S.aug_views()
    mg = AugMerge(2, 2, 'cuda', num_classes=3, nms_pre=1000, score_thr=0.05, iou_thr=0.3, nms_method=S.METHODS[method], soft_sigma=0.5,
                  soft_min_score=S.LONG_MIN_SCORE)
    for v, ((cls, raw, ctr), m) in enumerate(zip(views, metas)):
        vc = R.Case(cls, raw, ctr, 3, nms_pre=1000)
        dp = DetectPlan(1, sizes_of(vc), A.STRIDES[:2], 'cuda', num_classes=3, nms_pre=1000, ld_cls=4)
        bind(dp, vc)
        mg.collect(v, dp, m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'])
    dets, labels, count = mg.finish(True)
    torch.cuda.synchronize()
    k = int(count[0])
    assert k >= 0 and float(dets[0, k:].abs().sum()) == 0
    ref = S.aug(views, metas, 1000, 0.05, 0.3, 100, method, min_score=S.LONG_MIN_SCORE)
    n_decays = S.AUG_CLUSTER - 1                               # the pooled cluster is the largest class
    same((dets[0, :k].cpu(), labels[0, :k].cpu()), ref, S.score_rtol(n_decays, method))
    assert len(ref[0]) >= S.AUG_CLUSTER


def test_sweep_honours_test_cfg_soft_nms():
    """detect_device on a tiny network whose test_cfg asks for soft_nms: the detections are the model's on the head outputs the
    forward pass left in the plan's buffers (fp32 logits, so the network's bf16 noise is on both sides), not the hard NMS's - which
    is what the same call returned while the `type` key was dropped.  Criteria: aug_ref.match, the single-view parity test's."""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from dsl_amd.sweep import detect_device
    from oracle import fcos_oracle as O
    from util import fcos_model_cfg
    cfg = fcos_model_cfg()
    # The untrained head's boxes are a fraction of a stride wide and never overlap; a regression bias of 3 makes them about six
    # strides wide, so that neighbouring locations of a class overlap and the two NMS rules part.  max_per_img = 1000 shows the
    # decayed boxes that only Soft-NMS keeps.
    cfg['test_cfg'] = dict(cfg['test_cfg'], nms=dict(type='soft_nms', iou_threshold=0.3, min_score=1e-3), max_per_img=1000)
    sd = O.synth_state_dict(0)
    sd['bbox_head.conv_cls.bias'] = torch.full((80,), -2.5)
    sd['bbox_head.conv_reg.bias'] = torch.full((4,), 3.0)
    model = build_detector(cfg)
    model.load_state_dict(sd)
    model = model.cuda()
    n, H, W = 2, 64, 96
    img = (torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(9)) * 40).cuda()
    metas = [dict(img_shape=(H, W, 3), scale_factor=1.0)] * n
    dets, labels, count = detect_device(model, img, metas, rescale=False)
    torch.cuda.synchronize()
    plan = model._get_engine().plan(model.store, n, H, W, training=False)
    assert plan.detplan.desc.nms_method == S.METHODS['linear'] and plan.detplan.desc.soft_min_score == pytest.approx(1e-3)
    logits, regctr = plan.bufs['cls_logits'].float().cpu(), plan.bufs['regctr'].float().cpu()
    scales = [float(model.state_dict()[f'bbox_head.scales.{i}.scale']) for i in range(5)]
    cls, raw, ctr, m = [], [], [], 0
    for (h, w), sc in zip(plan.level_sizes, scales):
        rows = slice(m, m + n * h * w)
        lv = lambda t: t.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()      # noqa: E731
        cls.append(lv(logits[rows, :80]))
        raw.append(lv(regctr[rows, :4] * torch.tensor(sc)))
        ctr.append(lv(regctr[rows, 4:5]))
        m += n * h * w
    case = R.Case(cls, raw, ctr, 80, nms_pre=1000, max_per_img=1000, score_thr=0.05, iou_thr=0.3, img_shapes=[(H, W)] * n)
    differs = False
    for i, (ref, hard) in enumerate(zip(S.detect(case, 'linear', min_score=1e-3), R.detect(case))):
        k = int(count[i])
        print('image', i, 'kept', k, 'model', len(ref[0]), 'hard NMS', len(hard[0]), 'smallest gap of competing scores', S.min_gap(ref[2]))
        assert k >= 10
        A.match(dets[i, :k], labels[i, :k], ref[0].float(), ref[1])
        differs = differs or k != len(hard[0]) or not torch.allclose(dets[i, :k, 4].cpu(), hard[0][:, 4], rtol=1e-4)
    assert differs, 'the detections are the hard NMS\'s'
