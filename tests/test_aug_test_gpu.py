"""Test-time augmentation on the GPU: dsl_fcos_detect_collect / dsl_fcos_detect_finish against the reference's recorded
aug_test_bboxes outputs (tests/golden/aug_test_small.npz, made by tests/golden/make_aug_test.py) and against the single-view
dsl_fcos_detect.  Head outputs are bound straight into the detection plans, so the network's bf16 noise is not part of the
comparison.  Tolerances: aug_ref.match = the single-view parity test's (tests/test_sweep_gpu.py::_match)."""
import numpy as np
import pytest
import torch

import aug_ref as A
from util import fcos_model_cfg, levels_to_flat

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SIZES_A = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]          # 96 x 128
SHAPE_A = (96, 128, 3)
NMS_PRE = 50                                                  # level 0 of both views (192 / 96 locations) goes through the top-k
GUARD = 0x5A


def view_inputs(seed, C, sizes, exp_decode):
    return A.view_inputs(torch.Generator().manual_seed(seed), C, sizes, exp_decode)


def bound_plan(view, C, exp_decode, score_thr=0.05, guard=False):
    from dsl_amd import _lib as L
    from dsl_amd.params import HeadOptions
    from dsl_amd.sweep import DetectPlan
    cls, raw, ctr = view
    sizes = [tuple(c.shape[2:]) for c in cls]
    ld = (C + 3) // 4 * 4
    flat = levels_to_flat(cls)
    cls_f = torch.full((flat.shape[0], ld), 30.0)              # padding columns: a logit that would win if it were read
    cls_f[:, :C] = flat
    rc = torch.zeros(flat.shape[0], 8)
    rc[:, :4] = levels_to_flat(raw)
    rc[:, 4] = levels_to_flat(ctr)[:, 0]
    dp = DetectPlan(1, sizes, A.STRIDES, 'cuda', num_classes=C, nms_pre=NMS_PRE, ld_cls=ld, score_thr=score_thr,
                    head=HeadOptions(norm_on_bbox=False) if exp_decode else None)
    dp.bind(cls_f.cuda(), rc.cuda(), torch.ones(5, device='cuda'))
    if guard:          # guard words behind the view's own workspace, which collect writes as well
        need = dp.desc.workspace_bytes
        dp.ws = torch.full((need + 4096,), GUARD, dtype=torch.uint8, device='cuda')
        dp.desc.workspace = L.ptr(dp.ws)
    return dp


def run_aug(views, metas, C, exp_decode, rescale, score_thr=0.05, guard=False):
    from dsl_amd.sweep import AugMerge
    mg = AugMerge(len(views), 5, 'cuda', num_classes=C, nms_pre=NMS_PRE, score_thr=score_thr)
    if guard:          # guard words behind the queried size
        big = torch.full((mg.bytes + 4096,), GUARD, dtype=torch.uint8, device='cuda')
        mg.pool = big
    plans = [bound_plan(v, C, exp_decode, score_thr, guard) for v in views]
    for i, (dp, m) in enumerate(zip(plans, metas)):
        mg.collect(i, dp, m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'])
    dets, labels, count = mg.finish(rescale)
    torch.cuda.synchronize()
    k = int(count[0])
    if guard:
        assert bool((mg.pool[mg.bytes:] == GUARD).all()), 'written behind the queried pool size'
        for dp in plans:
            assert bool((dp.ws[dp.desc.workspace_bytes:] == GUARD).all()), 'written behind a view\'s queried workspace'
    assert k >= 0, 'finish reports a view missing from the pool'
    return dets[0, :k].cpu(), labels[0, :k].cpu()


def run_single(view, meta, C, exp_decode, score_thr=0.05):
    dp = bound_plan(view, C, exp_decode, score_thr)
    dp.set_meta([meta['img_shape']], [meta['scale_factor']], True)
    dp.run()
    torch.cuda.synchronize()
    k = int(dp.count[0])
    return dp.dets[0, :k].cpu(), dp.labels[0, :k].cpu()


def meta(shape, sf, direction=None):
    return dict(img_shape=shape, scale_factor=np.asarray(sf, np.float32), flip=direction is not None, flip_direction=direction)


@pytest.mark.parametrize('name', ['c80_tricks', 'c3_plain'])
@pytest.mark.parametrize('rescale', [True, False])
def test_fixture_parity_and_reproducible_bits(golden, name, rescale):
    """Views {A, A-hflip, B, B-vflip}, x / y scale factors unequal: the reference's detections, one to one; twice, the same bits."""
    d = golden('aug_test_small.npz')
    views, metas, C, exp_decode = A.fixture_views(d, name)
    assert int(d['nms_pre']) == NMS_PRE
    got_b, got_l = run_aug(views, metas, C, exp_decode, rescale, guard=True)
    ref_b = d[f'{name}_det_rescale' if rescale else f'{name}_det_norescale']
    print(name, rescale, 'kept', len(got_b), 'max |box - ref|', float((got_b[:, :4] - T(ref_b)[:len(got_b), :4]).abs().max()) if len(got_b) == len(ref_b) else None)
    A.match(got_b, got_l, ref_b, d[f'{name}_lab'])
    again_b, again_l = run_aug(views, metas, C, exp_decode, rescale)
    assert torch.equal(again_b, got_b) and torch.equal(again_l, got_l)


@pytest.mark.parametrize('C,exp_decode', [(80, False), (80, True), (3, False), (3, True)])
def test_duplicate_views_give_the_single_view_result(C, exp_decode):
    """[A, A]: every duplicate has IoU 1 with its twin and is suppressed; boxes, scores and labels are simple_test's, bit for bit."""
    view = view_inputs(7 + C, C, SIZES_A, exp_decode)
    m = meta(SHAPE_A, [1.25, 1.2, 1.25, 1.2])
    one_b, one_l = run_single(view, m, C, exp_decode)
    two_b, two_l = run_aug([view, view], [m, m], C, exp_decode, rescale=True, guard=True)
    assert len(one_b) >= 20
    assert torch.equal(two_b, one_b) and torch.equal(two_l, one_l)


SIZES_SQ = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]          # 128 x 128: every level's grid tiles the image in x AND y
SHAPE_SQ = (128, 128, 3)


@pytest.mark.parametrize('C,exp_decode,direction', [(80, False, 'horizontal'), (3, True, 'horizontal'), (80, True, 'vertical'),
                                                    (3, False, 'vertical'), (80, False, 'diagonal'), (3, True, 'diagonal')])
def test_flip_round_trip(C, exp_decode, direction):
    """[S, mirror(S)] with the head outputs mirrored accordingly: the mirrored view's candidates map back onto the plain view's and
    are suppressed by them.  S is 128 x 128, which all five strides divide, so every location of every level has its mirror image in
    every direction (96 x 128 would leave the rows of the 2 x 2 and 1 x 1 levels overhanging)."""
    cls, raw, ctr = view_inputs(11 + C, C, SIZES_SQ, exp_decode)
    mir = tuple(list(x) for x in zip(*[A.mirror(c, r, t, direction) for c, r, t in zip(cls, raw, ctr)]))
    sf = [1.25, 1.2, 1.25, 1.2]
    one_b, one_l = run_single((cls, raw, ctr), meta(SHAPE_SQ, sf), C, exp_decode)
    two_b, two_l = run_aug([(cls, raw, ctr), mir], [meta(SHAPE_SQ, sf), meta(SHAPE_SQ, sf, direction)], C, exp_decode, rescale=True,
                           guard=True)
    assert len(one_b) >= 20
    A.match(two_b, two_l, one_b, one_l)
    # and alone, the mirrored view gives the same detections as well
    mir_b, mir_l = run_aug([mir], [meta(SHAPE_SQ, sf, direction)], C, exp_decode, rescale=True)
    A.match(mir_b, mir_l, one_b, one_l)


def test_pool_cap_keeps_the_best_16384_pairs(golden):
    """score_thr = 0.001 makes ~31 000 of the four views' 31 680 pairs valid: the detections are the restatement's on the best
    16 384 pairs by final score, and nothing is written behind the queried pool."""
    d = golden('aug_test_small.npz')
    views, metas, C, exp_decode = A.fixture_views(d, 'c80_tricks')
    ref_b, ref_l, nvalid = A.aug_test_bboxes(views, metas, NMS_PRE, exp_decode, rescale=True, cap=16384, score_thr=0.001, iou_thr=0.5,
                                             max_per_img=100)
    assert nvalid > 16384 + 8000, nvalid
    got_b, got_l = run_aug(views, metas, C, exp_decode, True, score_thr=0.001, guard=True)
    A.match(got_b, got_l, ref_b, ref_l)


def test_finish_reports_a_view_that_was_not_collected():
    """A reused pool: finish consumes the views' records, so a second finish without new collects - or one view short - gives
    det_count = -1 and no detection instead of the previous image's rows; a view with another nms_pre is refused at its collect."""
    from dsl_amd.sweep import AugMerge
    view = view_inputs(5, 80, SIZES_A, False)
    m = meta(SHAPE_A, [1.0, 1.0, 1.0, 1.0])
    mg = AugMerge(2, 5, 'cuda', num_classes=80, nms_pre=NMS_PRE)
    dp = bound_plan(view, 80, False)

    def finish():
        _, _, count = mg.finish(True)
        torch.cuda.synchronize()
        return int(count[0])
    for v in (0, 1):
        mg.collect(v, dp, m['img_shape'], m['scale_factor'])
    assert finish() > 0
    assert finish() == -1                                   # consumed
    mg.collect(0, dp, m['img_shape'], m['scale_factor'])
    assert finish() == -1 and float(mg.dets.abs().sum()) == 0          # view 1 missing
    other = bound_plan(view, 80, False)
    other.desc.nms_pre = NMS_PRE - 10                       # would fit the pool's byte count, but is not the pool's
    mg.collect(0, dp, m['img_shape'], m['scale_factor'])
    with pytest.raises(RuntimeError, match='view 1 has .* nms_pre 40'):
        mg.collect(1, other, m['img_shape'], m['scale_factor'])
    assert finish() == -1                                   # view 1 still missing
    for v in (0, 1):
        mg.collect(v, dp, m['img_shape'], m['scale_factor'])
    assert finish() > 0


def test_existing_entry_keeps_its_bits(golden):
    """dsl_fcos_detect on test_sweep_gpu.py::test_detect_vs_reference_synth's inputs: the arrays recorded from the build before the
    collect / finish split (detect_bits_before_aug.npz), bit for bit."""
    from dsl_amd.sweep import DetectPlan
    d, want = golden('bboxes_synth.npz'), golden('detect_bits_before_aug.npz')
    sizes = [tuple(int(v) for v in s) for s in d['sizes']]
    cls = levels_to_flat([T(d[f'cls{i}']) for i in range(5)]).contiguous().cuda()
    rc = torch.zeros(cls.shape[0], 8)
    rc[:, :4] = levels_to_flat([T(d[f'reg{i}']) / s for i, s in zip(range(5), A.STRIDES)])
    rc[:, 4] = levels_to_flat([T(d[f'ctr{i}']) for i in range(5)])[:, 0]
    dp = DetectPlan(2, sizes, A.STRIDES, 'cuda')
    dp.bind(cls, rc.cuda(), torch.ones(5, device='cuda'))
    shp = tuple(int(x) for x in d['img_shape'])
    for rescale in (True, False):
        dp.set_meta([shp] * 2, [d['scale_factor']] * 2, rescale)
        dp.run()
        torch.cuda.synchronize()
        tag = 'rescale' if rescale else 'norescale'
        assert np.array_equal(dp.count.cpu().numpy(), want[f'count_{tag}'])
        assert np.array_equal(dp.dets.cpu().numpy().view(np.uint32), want[f'dets_{tag}'].view(np.uint32))
        assert np.array_equal(dp.labels.cpu().numpy(), want[f'labels_{tag}'])


def test_flipped_views_are_rendered_mirrored():
    """MultiScaleFlipAug through the image launch: each flipped view is the plain view of its scale, mirrored inside img_shape."""
    from dsl_amd.datapath import MultiScaleFlipAug
    TRANSFORMS = A.TRANSFORMS
    src = torch.randint(0, 256, (60, 90, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    aug = MultiScaleFlipAug(TRANSFORMS, img_scale=[(90, 60), (128, 96)], flip=True, flip_direction=['horizontal', 'vertical', 'diagonal'])
    out = aug(dict(img=src, filename='a.jpg'))
    torch.cuda.synchronize()
    assert len(out['img']) == 8 and all(len(m) == 1 for m in out['img_metas'])
    dims = {'horizontal': [3], 'vertical': [2], 'diagonal': [2, 3]}
    for base in (0, 4):
        plain, m0 = out['img'][base], out['img_metas'][base][0]
        h, w = m0['img_shape'][:2]
        assert plain.shape == (1, 3) + m0['pad_shape'][:2] and not m0['flip']
        for k in (1, 2, 3):
            img, m = out['img'][base + k], out['img_metas'][base + k][0]
            assert m['flip'] and m['img_shape'] == m0['img_shape']
            assert torch.equal(img[:, :, :h, :w], plain[:, :, :h, :w].flip(dims[m['flip_direction']]))
            assert float(img[:, :, h:].abs().sum()) == 0 and float(img[:, :, :, w:].abs().sum()) == 0


def test_end_to_end_four_views():
    """FCOS(return_loss=False, img=[4 views]) -> one list of num_classes (k, 5) arrays inside the original image; repeated calls
    allocate nothing; two images per view are refused.  (No comparison with the reference: the weights are random.)"""
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from oracle import fcos_oracle as O
    sd = O.synth_state_dict(0)
    sd['bbox_head.conv_cls.bias'] = torch.full((80,), -1.5)
    model = build_detector(fcos_model_cfg())
    model.load_state_dict(sd)
    model = model.cuda()
    g = torch.Generator().manual_seed(5)
    H, W = 96, 128
    shapes = [(96, 128), (96, 128), (64, 96), (64, 96)]
    flips = [None, 'horizontal', None, 'vertical']
    imgs = [(torch.randn(1, 3, h, w, generator=g) * 40).cuda() for h, w in shapes]
    metas = [[dict(img_shape=(h, w, 3), ori_shape=(H, W, 3), scale_factor=np.array([w / W, h / H, w / W, h / H], np.float32),
                   flip=f is not None, flip_direction=f)] for (h, w), f in zip(shapes, flips)]
    res = model(return_loss=False, rescale=True, img=imgs, img_metas=metas)
    assert isinstance(res, list) and len(res) == 1 and len(res[0]) == 80
    allb = np.concatenate(res[0])
    assert all(r.ndim == 2 and r.shape[1] == 5 for r in res[0]) and 0 < allb.shape[0] <= 100
    eps = 1e-3
    assert allb[:, [0, 2]].min() >= 0 and allb[:, [0, 2]].max() <= W + eps and allb[:, [1, 3]].min() >= 0 and allb[:, [1, 3]].max() <= H + eps
    assert (allb[:, 2] >= allb[:, 0]).all() and (allb[:, 3] >= allb[:, 1]).all()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        again = model(return_loss=False, rescale=True, img=imgs, img_metas=metas)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert all(np.array_equal(a, b) for a, b in zip(again[0], res[0]))
    # rescale=False: the same boxes in the first view's coordinates (its scale factor is 1 here)
    nores = model(return_loss=False, rescale=False, img=imgs, img_metas=metas)
    assert all(np.array_equal(a, b) for a, b in zip(nores[0], res[0]))
    with pytest.raises(ValueError, match='one image per view'):
        model(return_loss=False, img=[torch.cat([i, i]) for i in imgs], img_metas=[m + m for m in metas])
