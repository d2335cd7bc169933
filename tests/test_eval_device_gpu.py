"""The on-device evaluator (csrc/evalmap.hip through evaluation.coco_bbox_eval_device / eval_map_device / EvalHook(device_eval=True))
against the host path on the same inputs.  Every comparison is == / np.array_equal: the kernels restate the host's fp64 / fp32
operation order, so there is no tolerance anywhere in this file."""
import glob
import os

import numpy as np
import pytest
import torch

from util import fcos_model_cfg

pytestmark = pytest.mark.gpu

RANGES = ('all', 'small', 'medium', 'large')


def _ann(x, y, w, h, c, crowd=0, **kw):
    return dict(bbox=[x, y, w, h], category_id=c, iscrowd=crowd, **kw)


def _results(dets, img_ids, cat_ids):
    """(image_id, x, y, w, h, score, category_id) rows -> results[img][label] = (k, 5) float32 xyxy + score, rows in the given order."""
    out = [[[] for _ in cat_ids] for _ in img_ids]
    for i, x, y, w, h, s, c in dets:
        if c in cat_ids:
            out[img_ids.index(i)][cat_ids.index(c)].append([x, y, x + w, y + h, s])
    return [[np.asarray(b, np.float32).reshape(-1, 5) for b in r] for r in out]


def _both(results, img_ids, cat_ids, anns, **kw):
    from dsl_amd import evaluation as E
    host, hp = E.coco_bbox_eval(E.det2json(results, img_ids, cat_ids), img_ids, cat_ids, anns, return_precision=True, **kw)
    dev, dp = E.coco_bbox_eval_device(results, img_ids, cat_ids, anns, return_precision=True, **kw)
    return host, hp, dev, dp


def _check(results, img_ids, cat_ids, anns, **kw):
    host, hp, dev, dp = _both(results, img_ids, cat_ids, anns, **kw)
    for r in RANGES:
        assert dp[r].shape == hp[r].shape and dp[r].dtype == hp[r].dtype
        assert np.array_equal(dp[r], hp[r]), (r, np.argwhere(dp[r] != hp[r])[:5])
    assert list(dev.items()) == list(host.items())
    return host


# ---- 1. the constructed cases of tests/test_evaluation_cpu.py -------------------------------------------------------------------
def test_perfect_empty_and_category_without_ground_truth():
    anns = [[_ann(10, 10, 50, 50, 1), _ann(100, 100, 200, 200, 2)], [_ann(0, 0, 20, 20, 1)]]
    dets = [(1, 10, 10, 50, 50, .9, 1), (1, 100, 100, 200, 200, .8, 2), (2, 0, 0, 20, 20, .7, 1)]
    m = _check(_results(dets, [1, 2], [1, 2, 3]), [1, 2], [1, 2, 3], anns)
    assert m['mAP'] == pytest.approx(1.0) and m['mAP_s'] == pytest.approx(1.0) and m['mAP_l'] == pytest.approx(1.0)
    assert _check(_results([], [1, 2], [1, 2, 3]), [1, 2], [1, 2, 3], anns)['mAP'] == 0.0
    assert _check(_results(dets, [1, 2], [3]), [1, 2], [3], anns)['mAP'] == -1.0


def test_iou_thresholds():
    anns = [[_ann(0, 0, 100, 100, 1)]]
    assert _check(_results([(1, 10, 0, 100, 100, .9, 1)], [1], [1]), [1], [1], anns)['mAP'] == pytest.approx(0.7)
    m = _check(_results([(1, 30, 0, 100, 100, .9, 1)], [1], [1]), [1], [1], anns)      # IoU .538 counts only at .50
    assert m['mAP'] == pytest.approx(0.1) and m['mAP_75'] == 0.0


def test_ranking_duplicates_and_crowd():
    anns = [[_ann(0, 0, 50, 50, 1), _ann(200, 200, 50, 50, 1)]]
    want = (51 * 1.0 + 50 * (2 / 3)) / 101
    dets = [(1, 0, 0, 50, 50, .9, 1), (1, 400, 400, 50, 50, .8, 1), (1, 200, 200, 50, 50, .7, 1)]
    assert _check(_results(dets, [1], [1]), [1], [1], anns)['mAP_50'] == pytest.approx(want)
    dets = [(1, 0, 0, 50, 50, .9, 1), (1, 1, 0, 50, 50, .8, 1), (1, 200, 200, 50, 50, .7, 1)]
    assert _check(_results(dets, [1], [1]), [1], [1], anns)['mAP_50'] == pytest.approx(want)
    anns = [[_ann(0, 0, 50, 50, 1), _ann(100, 100, 300, 300, 1, crowd=1)]]
    dets = [(1, 150, 150, 40, 40, .95, 1), (1, 160, 160, 40, 40, .9, 1), (1, 0, 0, 50, 50, .5, 1)]
    assert _check(_results(dets, [1], [1]), [1], [1], anns)['mAP'] == pytest.approx(1.0)


def test_max_dets():
    anns = [[_ann(0, 0, 50, 50, 1)]]
    dets = [(1, 300 + i, 300, 10, 10, .9 - .001 * i, 1) for i in range(100)] + [(1, 0, 0, 50, 50, .1, 1)]
    res = _results(dets, [1], [1])
    assert _check(res, [1], [1], anns)['mAP'] == 0.0                       # the hit is detection 101
    assert _check(res, [1], [1], anns, max_dets=101)['mAP'] > 0.0


# ---- 2. exact-threshold ties ----------------------------------------------------------------------------------------------------
def test_iou_exactly_on_a_threshold():
    anns = [[_ann(0, 0, 100, 100, 1)], [_ann(0, 0, 100, 100, 1)]]
    dets = [(1, 0, 0, 100, 50, .9, 1), (2, 0, 0, 100, 75, .8, 1)]           # IoU exactly .5 and exactly .75
    m = _check(_results(dets, [1, 2], [1]), [1, 2], [1], anns)
    assert m['mAP_50'] == pytest.approx(1.0)


def test_equal_iou_candidates_and_regular_vs_crowd():
    # two ground-truth boxes with the same IoU to detection 1: the later one is taken (it is 'large' by its explicit area, so the
    # ranges see different matches); detection 2 then gets the earlier one
    anns = [[_ann(0, 0, 40, 40, 1), _ann(0, 0, 40, 40, 1, area=10000.0)],
            [_ann(0, 0, 60, 60, 1), _ann(20, 20, 80, 80, 1, crowd=1)]]
    dets = [(1, 0, 0, 40, 40, .9, 1), (1, 0, 0, 40, 40, .8, 1), (1, 1, 0, 40, 40, .7, 1),
            (2, 10, 10, 50, 50, .9, 1), (2, 25, 25, 30, 30, .8, 1), (2, 0, 0, 60, 60, .7, 1)]     # overlap a regular and a crowd box
    _check(_results(dets, [1, 2], [1]), [1, 2], [1], anns)


# ---- 3. seeded random sets ------------------------------------------------------------------------------------------------------
def _random_case(seed, big_gt=70, big_det=130):
    """6 images; categories 1, 2, 3 regular, 7 without ground truth, 9 without detections.  Scores are multiples of 1/8 (ties
    within cells and across images); areas straddle and sit on 32^2 / 96^2; some annotations carry `area`; 5 % crowd; cell
    (image 0, category 1) has `big_det` detections, cell (image 1, category 2) has `big_gt` ground-truth boxes."""
    rng = np.random.RandomState(seed)
    img_ids, cat_ids = [101, 102, 103, 104, 105, 106], [1, 2, 3, 7, 9]
    sizes = [(32., 32.), (96., 96.), (16., 64.), (48., 192.), (20., 20.), (50., 50.), (150., 120.), (31.5, 32.5), (96., 96.25)]

    def gt(c):
        w, h = sizes[rng.randint(len(sizes))]
        if rng.rand() < .4:
            w, h = w * rng.uniform(.7, 1.3), h * rng.uniform(.7, 1.3)
        a = _ann(float(rng.uniform(0, 400)), float(rng.uniform(0, 300)), float(w), float(h), c, crowd=int(rng.rand() < .05))
        if rng.rand() < .3:
            a['area'] = float(rng.choice([1024., 9216., w * h * .8, 500.]))
        return a

    def jitter(i, g, c):
        x, y, w, h = g['bbox']
        j = rng.normal(0, .1, 4) * [w, h, w, h] * (rng.rand() < .8)
        return (i, x + j[0], y + j[1], max(w + j[2], 2.), max(h + j[3], 2.), rng.randint(1, 9) / 8., c)

    anns, dets = [], []
    for k, i in enumerate(img_ids):
        a = [gt(c) for c in (1, 2, 3, 9) for _ in range(rng.randint(0, 4))]
        for g in a:
            if g['category_id'] != 9:
                dets += [jitter(i, g, g['category_id'] if rng.rand() < .85 else int(rng.choice([1, 2, 3, 7]))) for _ in range(rng.randint(0, 3))]
        if k == 1:
            fill = [gt(2) for _ in range(big_gt - sum(x['category_id'] == 2 for x in a))]
            dets += [jitter(i, g, 2) for g in fill[::4]]                  # the filling boxes: a detection for every fourth
            a += fill
        rng.shuffle(a)
        anns.append(a)
        dets += [(i, float(rng.uniform(0, 400)), float(rng.uniform(0, 300)), 30., 30., rng.randint(1, 9) / 8., int(rng.choice([1, 2, 3, 7])))
                 for _ in range(3)]
        if k == 0:
            own = [g for g in a if g['category_id'] == 1] or [_ann(50., 50., 40., 40., 1)]
            have = sum(d[0] == i and d[6] == 1 for d in dets)
            dets += [jitter(i, own[n % len(own)], 1) for n in range(big_det - have)]
    return _results(dets, img_ids, cat_ids), img_ids, cat_ids, anns


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_random_set_tables_and_metrics(seed):
    results, img_ids, cat_ids, anns = _random_case(seed)
    assert len(results[0][0]) == 130 and sum(a['category_id'] == 2 for a in anns[1]) == 70
    assert not any(len(r[4]) for r in results) and not any(a['category_id'] == 7 for x in anns for a in x)
    m = _check(results, img_ids, cat_ids, anns)
    assert 0.0 < m['mAP'] < 1.0


def test_more_ground_truth_than_the_lds_state_holds():
    """A cell with 140 ground-truth boxes keeps its matched flags in the workspace instead of LDS (the staging limit is 128)."""
    results, img_ids, cat_ids, anns = _random_case(3, big_gt=140, big_det=20)
    assert sum(a['category_id'] == 2 for a in anns[1]) == 140
    _check(results, img_ids, cat_ids, anns)


# ---- 4. the device triple and the list form -------------------------------------------------------------------------------------
def test_triple_and_list_forms_agree():
    from dsl_amd import evaluation as E
    results, img_ids, cat_ids, anns = _random_case(1, big_gt=10, big_det=10)
    K = max(sum(len(b) for b in r) for r in results) + 3
    dets, labels, count = np.zeros((len(results), K, 5), np.float32), np.zeros((len(results), K), np.int64), np.zeros(len(results), np.int32)
    for i, r in enumerate(results):
        lab = np.concatenate([np.full(len(b), c) for c, b in enumerate(r)])
        slot = np.argsort(-lab, kind='stable')          # classes in descending order, the rows of a class in their order
        count[i] = len(lab)
        dets[i, :len(lab)], labels[i, :len(lab)] = np.concatenate(r)[slot], lab[slot]
        dets[i, len(lab):, 4], labels[i, len(lab):] = 1.0, 0                                          # rows past count are not read
    triple = tuple(torch.from_numpy(a).cuda() for a in (dets, labels, count))
    a, pa = E.coco_bbox_eval_device(triple, img_ids, cat_ids, anns, return_precision=True)
    b, pb = E.coco_bbox_eval_device(results, img_ids, cat_ids, anns, return_precision=True)
    assert list(a.items()) == list(b.items()) and all(np.array_equal(pa[r], pb[r]) for r in RANGES)
    gt = E.flatten_annotations(anns, img_ids, cat_ids, 'coco')                                       # and with the cached ground truth
    assert list(E.coco_bbox_eval_device(triple, img_ids, cat_ids, gt).items()) == list(a.items())


# ---- 5. empty cases -------------------------------------------------------------------------------------------------------------
def test_no_detections_and_no_annotations():
    results, img_ids, cat_ids, anns = _random_case(2, big_gt=5, big_det=5)
    none = _results([], img_ids, cat_ids)
    assert _check(none, img_ids, cat_ids, anns)['mAP'] == 0.0
    assert _check(results, img_ids, cat_ids, [[] for _ in img_ids])['mAP'] == -1.0
    assert _check(none, img_ids, cat_ids, [[] for _ in img_ids])['mAP'] == -1.0
    torch.cuda.synchronize()


# ---- 6. VOC ---------------------------------------------------------------------------------------------------------------------
def _check_voc(results, anns, iou_thrs=(0.5, 0.75)):
    from dsl_amd import evaluation as E
    C = len(results[0])
    for thr in iou_thrs:
        # tp / fp per (image, class) against tpfp_default, in rank order (distinct scores: rank order is argsort(-score))
        p = E.pack_eval_inputs(*E._as_triple(results), anns, range(len(results)), range(C), 'voc', max_dets=None)
        tp, fp = (t.cpu().numpy() for t in E.voc_match_device(p, thr))
        off = p.det_off.cpu().numpy()
        for c in range(C):
            d, g, ig = E.get_cls_results(results, anns, c)
            for i in range(len(results)):
                t, f = E.tpfp_default(d[i], g[i], ig[i], thr)
                order = np.argsort(-d[i][:, 4], kind='stable')
                s0, s1 = off[c * len(results) + i], off[c * len(results) + i + 1]
                assert np.array_equal(tp[s0:s1], t[0][order].astype(np.uint8)), (thr, c, i)
                assert np.array_equal(fp[s0:s1], f[0][order].astype(np.uint8)), (thr, c, i)
        for dataset in ('voc07', None):
            hm, hr = E.eval_map(results, anns, iou_thr=thr, dataset=dataset)
            dm, dr = E.eval_map_device(results, anns, iou_thr=thr, dataset=dataset)
            assert dm == hm
            for a, b in zip(dr, hr):
                assert a['num_gts'] == b['num_gts'] and a['num_dets'] == b['num_dets'] and a['ap'] == b['ap'] and a['ap'].dtype == b['ap'].dtype
                assert np.array_equal(a['recall'], b['recall']) and np.array_equal(a['precision'], b['precision'])
    for year in (2007, 2012):
        host = E.voc_evaluate(results, anns, iou_thr=list(iou_thrs), year=year)
        assert list(E.voc_evaluate(results, anns, iou_thr=list(iou_thrs), year=year, device=True).items()) == list(host.items())


def test_voc_golden_inputs(golden):
    d = golden('voc_map.npz')
    n, C = int(d['n_img']), int(d['num_classes'])
    dets = [[d[f'det{i}_{c}'] for c in range(C)] for i in range(n)]
    anns = [{k: d[f'ann{i}_{k}'] for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore')} for i in range(n)]
    _check_voc(dets, anns)


@pytest.mark.parametrize('seed', [0, 1])
def test_voc_random_set_with_ignore_boxes(seed):
    """5 images x 4 classes, distinct scores (a shuffled linspace), ignore boxes - among them one that is a detection's first
    argmax and one that ties with a regular box listed before it - an image without any box, and one class with 150 boxes in
    an image (past the LDS staging limit)."""
    rng = np.random.RandomState(seed)
    N, C = 5, 4

    def boxes(n, lo=10, hi=120):
        xy = rng.uniform(0, 300, (n, 2))
        return np.hstack((xy, xy + rng.uniform(lo, hi, (n, 2)))).astype(np.float32)

    anns = []
    for i in range(N):
        n, k = (0, 0) if i == 2 else (rng.randint(3, 9), rng.randint(1, 4))
        anns.append(dict(bboxes=boxes(n), labels=rng.randint(0, C, n), bboxes_ignore=boxes(k), labels_ignore=rng.randint(0, C, k)))
    anns[3]['bboxes'] = np.vstack((anns[3]['bboxes'], boxes(150, 10, 40)))
    anns[3]['labels'] = np.concatenate((anns[3]['labels'], np.full(150, 1)))
    anns[0]['bboxes_ignore'] = np.vstack((anns[0]['bboxes_ignore'], anns[0]['bboxes'][:1]))        # ties with regular box 0: the regular one is first
    anns[0]['labels_ignore'] = np.concatenate((anns[0]['labels_ignore'], anns[0]['labels'][:1]))
    per = [[[] for _ in range(C)] for _ in range(N)]
    for i, a in enumerate(anns):
        for b, l in list(zip(a['bboxes'][:12], a['labels'][:12])) + list(zip(a['bboxes_ignore'], a['labels_ignore'])):
            for _ in range(rng.randint(1, 4)):                         # jittered copies: hits, duplicates of a covered box, misses
                j = rng.normal(0, .15, 4) * np.tile(b[2:] - b[:2], 2) * (rng.rand() < .7)
                per[i][int(l)].append(b + j.astype(np.float32))
        for _ in range(3):
            per[i][rng.randint(C)].append(boxes(1)[0])
    total = sum(len(c) for r in per for c in r)
    scores = iter(rng.permutation(np.linspace(.05, .95, total)).astype(np.float32))
    results = [[np.array([np.append(b, next(scores)) for b in c], np.float32).reshape(-1, 5) for c in r] for r in per]
    assert len(set(np.concatenate([c[:, 4] for r in results for c in r]).tolist())) == total
    _check_voc(results, anns, iou_thrs=(0.5, 0.55))


# ---- 7. EvalHook(device_eval=True) ----------------------------------------------------------------------------------------------
def _model():
    from dsl_amd import detectors  # noqa: F401
    from dsl_amd.registry import build_detector
    from oracle import fcos_oracle as O
    m = build_detector(fcos_model_cfg())
    sd = O.synth_state_dict(0)
    sd['bbox_head.conv_cls.bias'] = torch.full_like(sd['bbox_head.conv_cls.bias'], 0.0)      # scores above score_thr: detections exist
    m.load_state_dict(sd)
    return m.cuda()


@pytest.mark.parametrize('metric', ['bbox', 'mAP'])
def test_eval_hook_device_eval_returns_the_default_hooks_metrics(tmp_path, metric):
    from dsl_amd import evaluation as E
    from dsl_amd.data import SyntheticValLoader
    from dsl_amd.runner import SemiEpochBasedRunner
    det = _model()
    loader = SyntheticValLoader(n_images=3, H=128, W=192, W_img=190)
    work_host, work_dev = tmp_path / 'host', tmp_path / 'dev'
    r_host = SemiEpochBasedRunner(det, optimizer=None, max_epochs=1, work_dir=str(work_host))
    r_dev = SemiEpochBasedRunner(det, optimizer=None, max_epochs=1, work_dir=str(work_dev))
    want = E.EvalHook(loader, metric=metric)._do_evaluate(r_host)
    hook = E.EvalHook(loader, metric=metric, device_eval=True)
    got = hook._do_evaluate(r_dev)
    assert list(got.items()) == list(want.items()) and hook.history == [(1, dict(want))]
    assert not glob.glob(os.path.join(str(work_dev), '**', '*.json'), recursive=True)           # no prefix given: no json
    if metric == 'bbox':
        assert sum(E.triple_to_results(E.single_gpu_test(det, loader, keep_on_device=True), 80)[i][c].shape[0]
                   for i in range(3) for c in range(80)) > 0
        prefix = str(tmp_path / 'explicit' / 'val')
        assert list(E.EvalHook(loader, metric=metric, device_eval=True, jsonfile_prefix=prefix)._do_evaluate(r_dev).items()) == list(want.items())
        assert os.path.exists(prefix + '.bbox.json')
