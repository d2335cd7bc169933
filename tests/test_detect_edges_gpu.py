"""dsl_fcos_detect, dsl_fcos_detect_collect / _finish and pseudo_fuse_kernel on structured inputs - ties, caps, thresholds that are
hit exactly, empty images - against tests/detect_ref.py (the fp32 model with the kernel's documented tie rules) and
dsl_amd.pseudo.fuse_host.  tests/test_detect_edges_cpu.py proves what each input hits.  Count, labels and order must match exactly,
scores and boxes to test_sweep_gpu.py::_match's tolerances, and nothing is ordered 'up to ties' before it is compared."""
import numpy as np
import pytest
import torch

import detect_ref as R
import fuse_cases as F
from util import levels_to_flat

pytestmark = pytest.mark.gpu
PAD = 50.0                                                    # logit of the padding columns of a row: it would win if it were read


def make_plan(case):
    from dsl_amd.sweep import DetectPlan
    ld = (case.C + 4) // 4 * 4                                # at least one padding column
    return DetectPlan(case.n, R.SIZES, R.STRIDES, 'cuda', num_classes=case.C, nms_pre=case.nms_pre, max_per_img=case.max_per_img,
                      score_thr=case.score_thr, iou_thr=case.iou_thr, ld_cls=ld)


def bind(dp, case):
    f = levels_to_flat(case.cls)
    cls = torch.full((f.shape[0], dp.desc.ld_cls), PAD)
    cls[:, :case.C] = f
    rc = torch.zeros(f.shape[0], 8)
    rc[:, :4] = levels_to_flat(case.raw)
    rc[:, 4] = levels_to_flat(case.ctr)[:, 0]
    dp.bind(cls.cuda(), rc.cuda(), torch.ones(5, device='cuda'))
    dp.set_meta(case.img_shapes, case.scale_factors, case.rescale)


def run(case, dp=None):
    """Per image (dets [k, 5], labels [k]) on the host; the rows behind the count must be zero."""
    dp = dp or make_plan(case)
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


def same(got, ref, what=''):
    (gb, gl), (rb, rl) = got, ref[:2]
    print(what, 'kept', len(gb), 'reference', len(rb))
    assert len(gb) == len(rb), (len(gb), len(rb))
    assert torch.equal(gl, rl)
    if len(gb):
        print(what, 'max |score - ref|', float((gb[:, 4] - rb[:, 4]).abs().max()), 'max |box - ref|', float((gb[:, :4] - rb[:, :4]).abs().max()))
    assert torch.allclose(gb[:, 4], rb[:, 4], rtol=1e-4, atol=1e-6)
    assert torch.allclose(gb[:, :4], rb[:, :4], rtol=1e-4, atol=1e-3)
    # identical inputs give identical bits: every group of equal reference scores is one bit pattern on the device as well
    for v in rb[:, 4].unique():
        assert len(gb[rb[:, 4] == v, 4].unique()) == 1


def check(case):
    for i, (g, r) in enumerate(zip(run(case), R.detect(case))):
        same(g, r, f'image {i}')


@pytest.mark.parametrize('which', ['within_first', 'beyond_first', 'third', 'both_select'])
def test_topk_ties_across_wave_segments(which):
    """The k-th key's tie group is cut inside, in the first / second / third 256-element segment of ordered_compact (both_select:
    on two levels, next to three levels that are taken whole): the lowest indices are taken."""
    check(R.topk_ties(which))


def test_all_keys_equal():
    check(R.all_equal())


@pytest.mark.parametrize('which,max_per_img', [('one', 20), ('one', 1024), ('all', 1024)])
def test_fewer_positive_keys_than_nms_pre(which, max_per_img):
    """All positive keys plus the lowest-index zero keys; a pair whose class score is above score_thr and whose centerness sigmoid is 0
    is valid with final score 0 (bbox_nms.py tests validity before the centerness factor) and is emitted when fewer than max_per_img
    boxes survive."""
    case = R.few_positive(which, max_per_img)
    got = run(case)[0]
    same(got, R.detect(case)[0])
    assert int((got[0][:, 4] == 0).sum()) == {('one', 20): 0, ('one', 1024): 1, ('all', 1024): 161}[which, max_per_img]


@pytest.mark.parametrize('which,max_per_img', [('distinct', 100), ('zeros', 1024)])
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_candidate_count_at_the_path_switch(delta, which, max_per_img):
    """CAND_CAP - 1, CAND_CAP (64-chunk count / scatter) and CAND_CAP + 1 (single-block best-CAND_CAP) valid pairs."""
    check(R.at_cap(delta, which, max_per_img))


@pytest.mark.parametrize('delta', [-1, 0, 1, 2000])
def test_tie_group_at_the_cap(delta):
    """One group of equal final scores behind 40 distinct ones, CAND_CAP + delta valid pairs; the group's members that the NMS does
    not suppress lie on both sides of the cut and the output runs up to it (max_per_img = survivors inside the cap - 1): the cut
    keeps the lowest candidate numbers.  2000: members on both sides of the cut in several wave segments of det_compact_kernel."""
    check(R.at_cap(delta, 'tied'))


def test_score_ties_through_sort_and_nms():
    check(R.score_ties())


@pytest.mark.parametrize('score_thr', [0.5, R.BELOW_HALF])
def test_thresholds_are_strict(score_thr):
    """score 0.5f is invalid at score_thr 0.5 and valid one ulp below; IoU 0.5 at iou_thr 0.5 keeps both boxes, 0.5625 suppresses,
    and not across classes.  Integer boxes and max + 1 = 161: the fp32 class offset is exact (detect_ref.thresholds)."""
    case = R.thresholds(score_thr)
    got = run(case)[0]
    same(got, R.detect(case)[0])
    assert got[1].tolist() == [7, 7, 7, 7, 3] + ([] if score_thr == 0.5 else [1, 1])


def test_degenerate_boxes():
    check(R.degenerate())


@pytest.mark.parametrize('rescale', [True, False])
def test_batch_edges_and_no_state_between_slots_or_runs(rescale):
    """n = 3 - empty, one pair, full - with three img_shapes and non-uniform 4-component scale factors; then the same plan on the
    images in another order, and back: every image's detections keep their bits whichever slot and run they are in."""
    case = R.batch(rescale)
    dp = make_plan(case)
    first = run(case, dp)
    for i, (g, r) in enumerate(zip(first, R.detect(case))):
        same(g, r, f'image {i}')
    assert len(first[0][0]) == 0 and len(first[1][0]) == 1 and len(first[2][0]) == case.max_per_img
    order = [2, 0, 1]
    moved = run(case.permuted(order), dp)
    for slot, i in enumerate(order):
        assert torch.equal(moved[slot][0], first[i][0]) and torch.equal(moved[slot][1], first[i][1])
    again = run(case, dp)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(again, first))


@pytest.mark.parametrize('max_per_img', [1, R.NMS_THREADS])
@pytest.mark.parametrize('C', [1, 3, 80])
def test_max_per_img_edges(C, max_per_img):
    """More survivors than max_per_img = 1 and = NMS_THREADS; num_classes 1, 3, 80 with padding columns at +50 behind them.  (C == 1:
    one pair per location, so exactly 1 024 survivors - the limit of 1 024 is met, not exceeded; C = 3 and 80 have 2 048.)"""
    check(R.many_survivors(C, max_per_img))


def test_max_per_img_above_nms_threads_is_refused():
    case = R.many_survivors(3, R.NMS_THREADS + 1)
    dp = make_plan(case)
    bind(dp, case)
    with pytest.raises(RuntimeError, match='max_per_img must be in 1..1024'):
        dp.run()


# ---- the same pools through collect / finish --------------------------------------------------------------------------------------
def run_aug(views):
    from dsl_amd.sweep import AugMerge
    v0 = views[0]
    mg = AugMerge(len(views), 5, 'cuda', num_classes=v0.C, nms_pre=v0.nms_pre, max_per_img=v0.max_per_img, score_thr=v0.score_thr,
                  iou_thr=v0.iou_thr)
    plans = [make_plan(v) for v in views]
    for i, (dp, v) in enumerate(zip(plans, views)):
        bind(dp, v)
        mg.collect(i, dp, R.SHAPE + (3,), np.ones(4, np.float32))
    dets, labels, count = mg.finish(True)
    torch.cuda.synchronize()
    k = int(count[0])
    assert k >= 0 and float(dets[0, k:].abs().sum()) == 0
    return dets[0, :k].cpu(), labels[0, :k].cpu()


def test_collect_finish_tie_at_the_cap():
    views = R.aug_tie_at_cap()
    same(run_aug(views), R.aug_ref(views))


def test_collect_finish_empty_image():
    got = run_aug(R.aug_empty())
    assert len(got[0]) == 0
    same(got, R.aug_ref(R.aug_empty()))


# ---- pseudo_fuse_kernel -----------------------------------------------------------------------------------------------------------
def run_fuse(imgs, maxk, parse, iou, counts=None, olds=None, max_old=0, old_counts=None):
    """imgs: [(dets [k, 5], labels [k])] per image; olds: per image the stored labels (fuse_host's `old`).  Returns per image
    dict(rects, tags, scores), and checks it against fuse_host on what the kernel may read: the first min(count, maxk) detections
    and min(old_count, max_old) stored labels."""
    from dsl_amd import _lib as L
    from dsl_amd.pseudo import fuse_host
    n = len(imgs)
    dets, labels = torch.zeros(n, maxk, 5), torch.zeros(n, maxk, dtype=torch.int64)
    for i, (d, l) in enumerate(imgs):
        k = min(len(d), maxk)
        dets[i, :k], labels[i, :k] = torch.from_numpy(d[:k]), torch.from_numpy(l[:k])
    counts = counts or [len(d) for d, _ in imgs]
    mo = max(max_old, 1)
    ob_, os_, ol_ = torch.zeros(n, mo, 4), torch.zeros(n, mo), torch.zeros(n, mo, dtype=torch.int64)
    old_counts = old_counts or [len(o['scores']) if o else 0 for o in (olds or [None] * n)]
    for i, o in enumerate(olds or []):
        if o:
            k = min(len(o['scores']), max_old)
            ob_[i, :k], os_[i, :k], ol_[i, :k] = (torch.from_numpy(o[key][:k]) for key in ('rects', 'scores', 'tags'))
    mout = max_old + maxk
    dev = [t.cuda() for t in (dets, labels, torch.tensor(counts, dtype=torch.int32), ob_, os_, ol_, torch.tensor(old_counts, dtype=torch.int32))]
    ob, osc = torch.full((n, mout, 4), -7.0, device='cuda'), torch.full((n, mout), -7.0, device='cuda')
    ol, oc = torch.full((n, mout), -7, dtype=torch.int64, device='cuda'), torch.full((n,), -7, dtype=torch.int32, device='cuda')
    L.check(L.lib.dsl_pseudo_label_fuse_history(L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), n, maxk, L.ptr(dev[3]), L.ptr(dev[4]),
                                                L.ptr(dev[5]), L.ptr(dev[6]), max_old, F.C, parse, iou, F.NMS_THR, L.ptr(ob), L.ptr(osc),
                                                L.ptr(ol), L.ptr(oc), mout, L.stream_ptr()), 'dsl_pseudo_label_fuse_history')
    torch.cuda.synchronize()
    out = []
    for i, (d, l) in enumerate(imgs):
        k, ko = min(counts[i], maxk), min(old_counts[i], max_old)
        old = {key: olds[i][key][:ko] for key in ('rects', 'tags', 'scores')} if ko else None
        ref = fuse_host(d[:k], l[:k], parse, iou, F.NMS_THR, F.C, old=old)
        m = int(oc[i])
        got = dict(rects=ob[i, :m].cpu().numpy(), tags=ol[i, :m].cpu().numpy(), scores=osc[i, :m].cpu().numpy())
        print('image', i, 'fused', m, 'host', len(ref['tags']))
        assert m == len(ref['tags'])
        assert np.array_equal(got['tags'], ref['tags']) and np.array_equal(got['rects'], ref['rects'])
        assert np.array_equal(got['scores'].view(np.uint32), ref['scores'].view(np.uint32))
        out.append(got)
    return out


def test_fuse_rounding_ties_keep_the_earlier_detection_first():
    d, l = F.rounding_ties()
    out = run_fuse([(d, l)], 100, F.PARSE, 0.5)[0]
    assert out['rects'][1:3].tolist() == np.trunc(d[:2, :4]).tolist() and out['scores'][1] == out['scores'][2] == np.float32(0.4)


def test_fuse_threshold_rules():
    d, l = F.threshold_rules()
    assert len(run_fuse([(d, l)], 100, F.PARSE, 0.5)[0]['tags']) == 1          # score == parse_thr is kept, one ulp below is not
    assert len(run_fuse([(d, l)], 100, 0.05, 0.5)[0]['tags']) == 2             # a rounded score == nms_thr is dropped


def test_fuse_truncates_toward_zero():
    d, l = F.truncation()
    out = run_fuse([(d, l)], 100, F.PARSE, 0.5)[0]
    assert out['rects'].tolist() == [[0, 0, 16, 16], [0, 0, 16, 8], [-3, -2, 10, 7]]       # IoU of the first two == iou_thr: both kept


def test_fuse_drops_labels_out_of_range():
    d, l = F.label_range()
    assert run_fuse([(d, l)], 100, F.PARSE, 0.5)[0]['tags'].tolist() == [0, F.C - 1]


def test_fuse_count_edges():
    """Five images in one launch: count above max_per_img (clamped), 0, 1, full, and a few; with history - stored labels at exactly
    max_old, above it (clamped), none - and max_old + max_per_img == 1024."""
    maxk, max_old = 100, 924
    imgs = [F.random_dets(1, 100), F.random_dets(2, 100), F.random_dets(3, 1), F.random_dets(4, 100), F.random_dets(5, 7)]
    counts = [105, 0, 1, 100, 7]
    run_fuse(imgs, maxk, 0.2, 0.6, counts=counts)
    olds = [F.random_old(11, 924), F.random_old(12, 924), None, F.random_old(13, 40), None]
    run_fuse(imgs, maxk, 0.2, 0.6, counts=counts, olds=olds, max_old=max_old, old_counts=[924, 930, 0, 40, 0])
