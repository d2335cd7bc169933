"""Evaluation / interop side of the detector:

  results2json / format_results   mmdet/datasets/coco.py:179-360 (COCO detection-result json: xywh boxes, category ids)
  single_gpu_test / multi_gpu_test mmdet/apis/test.py (the loops EvalHook drives); detections come from the HIP sweep
  EvalHook                         mmdet/core/evaluation/eval_hooks.py:9-66: evaluates the EMA teacher once it exists
                                   (DistEvalHook :24-66 `if runner.ema_flag: model = runner.ema_model`), every `interval` epochs
  coco_bbox_eval                   the bbox protocol of pycocotools' COCOeval (10 IoU thresholds .50:.05:.95, 101 recall points,
                                   maxDets 100, crowd = ignore, area ranges) restated in numpy - pycocotools is not in this
                                   image, so this evaluator is checked on constructed cases only: PARITY UNPINNED against
                                   pycocotools; the json files are the interop path to the real tool.

  eval_map / VOCEvalDataset       mmdet/core/evaluation/mean_ap.py (average_precision, tpfp_default, get_cls_results, eval_map)
                                   and VOCDataset.evaluate(metric='mAP') (mmdet/datasets/voc.py:27-90), in-process numpy;
                                   pinned to the reference by tests/golden/voc_map.npz.

The dataset side is a plain object (or dict) with `img_ids`, `cat_ids` and, for the built-in evaluator, `annotations`:
one list per image of dict(bbox=[x, y, w, h], category_id, iscrowd=0, area=optional).  With `metric='mAP'` (the VOC configs'
`evaluation = dict(metric='mAP')`) the annotations are instead one dict per image of `bboxes` [n, 4] xyxy, `labels` [n] (0-based),
`bboxes_ignore` [k, 4], `labels_ignore` [k], and an optional `year` (2007 selects VOC07's 11-point AP).
"""
import json
import os
import tempfile
from collections import OrderedDict

import numpy as np
import torch


def xyxy2xywh(bbox):
    """coco.py:179-196."""
    b = np.asarray(bbox).tolist()
    return [b[0], b[1], b[2] - b[0], b[3] - b[1]]


def det2json(results, img_ids, cat_ids):
    """coco.py:213-229 (_det2json): results[idx][label] = ndarray (k, 5) xyxy + score."""
    out = []
    for idx, img_id in enumerate(img_ids):
        for label, bboxes in enumerate(results[idx]):
            for i in range(bboxes.shape[0]):
                out.append(dict(image_id=img_id, bbox=xyxy2xywh(bboxes[i]), score=float(bboxes[i][4]), category_id=cat_ids[label]))
    return out


def results2json(results, img_ids, cat_ids, outfile_prefix):
    """coco.py:269-304 for detection results: writes <prefix>.bbox.json, returns {'bbox': path, 'proposal': path}."""
    if not isinstance(results[0], list):
        raise TypeError('invalid type of results')
    files = dict(bbox=f'{outfile_prefix}.bbox.json', proposal=f'{outfile_prefix}.bbox.json')
    os.makedirs(os.path.dirname(os.path.abspath(files['bbox'])), exist_ok=True)
    with open(files['bbox'], 'w') as f:
        json.dump(det2json(results, img_ids, cat_ids), f)
    return files


def format_results(results, img_ids, cat_ids, jsonfile_prefix=None):
    """coco.py:334-360."""
    assert isinstance(results, list), 'results must be a list'
    assert len(results) == len(img_ids), f'The length of results is not equal to the dataset len: {len(results)} != {len(img_ids)}'
    tmp_dir = None
    if jsonfile_prefix is None:
        tmp_dir = tempfile.TemporaryDirectory()
        jsonfile_prefix = os.path.join(tmp_dir.name, 'results')
    return results2json(results, img_ids, cat_ids, jsonfile_prefix), tmp_dir


# ----------------------------------------------------------------------------------------------------------------------
def _iou_xywh(d, g, crowd):
    """[D, G] IoU of xywh boxes; against a crowd box the union is the detection's area (COCO maskUtils.iou)."""
    d, g = np.asarray(d, np.float64).reshape(-1, 4), np.asarray(g, np.float64).reshape(-1, 4)
    if not len(d) or not len(g):
        return np.zeros((len(d), len(g)))
    dx2, dy2, gx2, gy2 = d[:, 0] + d[:, 2], d[:, 1] + d[:, 3], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    iw = np.clip(np.minimum(dx2[:, None], gx2[None]) - np.maximum(d[:, None, 0], g[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(dy2[:, None], gy2[None]) - np.maximum(d[:, None, 1], g[None, :, 1]), 0, None)
    inter = iw * ih
    da, ga = (d[:, 2] * d[:, 3])[:, None], (g[:, 2] * g[:, 3])[None]
    union = np.where(np.asarray(crowd, bool)[None], da, da + ga - inter)
    return inter / np.maximum(union, 1e-12)


COCO_AREA_RANGES = OrderedDict(all=(0, 1e10), small=(0, 32 ** 2), medium=(32 ** 2, 96 ** 2), large=(96 ** 2, 1e10))


def coco_bbox_eval(dets, img_ids, cat_ids, annotations, iou_thrs=None, max_dets=100, return_precision=False):
    """dets: the list det2json produces; annotations[idx]: list of dict(bbox xywh, category_id, iscrowd, [area]).
    Returns OrderedDict(mAP, mAP_50, mAP_75, mAP_s, mAP_m, mAP_l) (-1 where no ground truth falls in the range); with
    `return_precision` also {range: [T, 101, C] precision table}."""
    iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    rec_thrs = np.linspace(0, 1, 101)
    ranges = COCO_AREA_RANGES
    by = {}
    for d in dets:
        by.setdefault((d['image_id'], d['category_id']), []).append(d)
    prec = {r: -np.ones((len(iou_thrs), len(rec_thrs), len(cat_ids))) for r in ranges}
    for ci, cat in enumerate(cat_ids):
        for rname, (lo, hi) in ranges.items():
            scores, matched, ignored, npos = [], [], [], 0
            for idx, img_id in enumerate(img_ids):
                gts = [a for a in annotations[idx] if a['category_id'] == cat]
                garea = np.array([a.get('area', a['bbox'][2] * a['bbox'][3]) for a in gts], np.float64)
                crowd = np.array([bool(a.get('iscrowd', 0)) for a in gts], bool)
                gig = crowd | (garea < lo) | (garea > hi)
                order = np.argsort(gig, kind='mergesort')            # non-ignored ground truth first
                gts, crowd, gig = [gts[i] for i in order], crowd[order], gig[order]
                dd = sorted(by.get((img_id, cat), []), key=lambda d: -d['score'])[:max_dets]
                ious = _iou_xywh([d['bbox'] for d in dd], [a['bbox'] for a in gts], crowd)
                npos += int((~gig).sum())
                dm = -np.ones((len(iou_thrs), len(dd)), int)
                dig = np.zeros((len(iou_thrs), len(dd)), bool)
                for ti, t in enumerate(iou_thrs):
                    gm = -np.ones(len(gts), int)
                    for di in range(len(dd)):
                        best, m = min(t, 1 - 1e-10), -1
                        for gi in range(len(gts)):
                            if gm[gi] >= 0 and not crowd[gi]:
                                continue
                            if m > -1 and not gig[m] and gig[gi]:
                                break                                  # already matched to a regular gt: do not trade it for an ignored one
                            if ious[di, gi] < best:
                                continue
                            best, m = ious[di, gi], gi
                        if m >= 0:
                            dm[ti, di], gm[m], dig[ti, di] = m, di, gig[m]
                darea = np.array([d['bbox'][2] * d['bbox'][3] for d in dd], np.float64)
                dig |= (dm < 0) & ((darea < lo) | (darea > hi))[None]
                scores += [d['score'] for d in dd]
                matched.append(dm >= 0)
                ignored.append(dig)
            if npos == 0:
                continue
            sc = np.array(scores)
            order = np.argsort(-sc, kind='mergesort')
            mt = np.concatenate(matched, 1)[:, order] if matched else np.zeros((len(iou_thrs), 0), bool)
            ig = np.concatenate(ignored, 1)[:, order] if ignored else np.zeros((len(iou_thrs), 0), bool)
            for ti in range(len(iou_thrs)):
                tp = np.cumsum(mt[ti] & ~ig[ti])
                fp = np.cumsum(~mt[ti] & ~ig[ti])
                rc = tp / npos
                pr = tp / np.maximum(tp + fp, np.spacing(1))
                for i in range(len(pr) - 1, 0, -1):                    # precision envelope
                    pr[i - 1] = max(pr[i - 1], pr[i])
                q = np.zeros(len(rec_thrs))
                inds = np.searchsorted(rc, rec_thrs, side='left')
                ok = inds < len(pr)
                q[ok] = pr[inds[ok]]
                prec[rname][ti, :, ci] = q

    metrics = _coco_summary(prec, iou_thrs)
    return (metrics, prec) if return_precision else metrics


def _coco_summary(prec, iou_thrs):
    """The closing means of coco_bbox_eval over prec[range] = [T, 101, C] (-1 = no ground truth): shared by the host and the
    device evaluator, so that numpy sums the same arrays in the same order."""
    def mean(p, ti=None):
        p = p if ti is None else p[ti:ti + 1]
        v = p[p > -1]
        return float(v.mean()) if v.size else -1.0
    i50 = int(np.argmin(np.abs(iou_thrs - .5)))
    i75 = int(np.argmin(np.abs(iou_thrs - .75)))
    return OrderedDict(mAP=mean(prec['all']), mAP_50=mean(prec['all'], i50), mAP_75=mean(prec['all'], i75), mAP_s=mean(prec['small']),
                       mAP_m=mean(prec['medium']), mAP_l=mean(prec['large']))


# ----------------------------------------------------------------------------------------------------------------------
# PASCAL VOC mAP (mean_ap.py): per class, detections of all images sorted by score, greedy matching per image at one IoU
def average_precision(recalls, precisions, mode='area'):
    """AP of one or several (num_scales rows) precision / recall curves: 'area' = area under the precision envelope,
    '11points' = mean of the best precision at recall >= 0, 0.1, ..., 1 (VOC07)."""
    rec, prec = np.asarray(recalls), np.asarray(precisions)
    single = rec.ndim == 1
    rec, prec = np.atleast_2d(rec), np.atleast_2d(prec)
    assert rec.shape == prec.shape
    ap = np.zeros(rec.shape[0], dtype=np.float32)
    if mode == 'area':
        for i in range(rec.shape[0]):
            r = np.concatenate(([0.], rec[i], [1.])).astype(rec.dtype)
            p = np.concatenate(([0.], prec[i], [0.])).astype(prec.dtype)
            p = np.maximum.accumulate(p[::-1])[::-1]                  # precision envelope
            step = np.nonzero(r[1:] != r[:-1])[0]
            ap[i] = np.sum((r[step + 1] - r[step]) * p[step + 1])
    elif mode == '11points':
        for i in range(rec.shape[0]):
            for t in np.arange(0, 1 + 1e-3, 0.1):
                sel = prec[i, rec[i] >= t]
                ap[i] += sel.max() if sel.size else 0
        ap /= 11
    else:
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    return ap[0] if single else ap


def _overlaps(a, b):
    """[n, k] IoU of xyxy boxes in float32 (evaluation/bbox_overlaps.py: no +1, union clamped at 1e-6)."""
    a, b = np.asarray(a, np.float32).reshape(-1, 4), np.asarray(b, np.float32).reshape(-1, 4)
    if not len(a) or not len(b):
        return np.zeros((len(a), len(b)), np.float32)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0)
    ih = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0)
    inter = iw * ih
    return inter / np.maximum(area_a[:, None] + area_b[None] - inter, np.float32(1e-6))


def tpfp_default(det_bboxes, gt_bboxes, gt_bboxes_ignore=None, iou_thr=0.5, area_ranges=None):
    """(tp, fp), each [num_scales, num_dets] float32, for one image and class.  A detection whose best-IoU ground truth
    (>= iou_thr) is an ignore box or out of the area range counts as neither; a second detection of a covered box is a false
    positive; an unmatched detection is a false positive when its own area is inside the range."""
    det = np.asarray(det_bboxes, np.float32).reshape(-1, 5)
    gt = np.asarray(gt_bboxes, np.float32).reshape(-1, 4)
    ig = np.zeros((0, 4), np.float32) if gt_bboxes_ignore is None else np.asarray(gt_bboxes_ignore, np.float32).reshape(-1, 4)
    is_ig = np.concatenate((np.zeros(len(gt), bool), np.ones(len(ig), bool)))
    allgt = np.vstack((gt, ig))
    ranges = [(None, None)] if area_ranges is None else list(area_ranges)
    tp = np.zeros((len(ranges), len(det)), np.float32)
    fp = np.zeros((len(ranges), len(det)), np.float32)
    det_area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    if len(allgt) == 0:
        for k, (lo, hi) in enumerate(ranges):
            fp[k] = 1 if lo is None else ((det_area >= lo) & (det_area < hi))
        return tp, fp
    ious = _overlaps(det[:, :4], allgt)
    best, arg = ious.max(axis=1), ious.argmax(axis=1)
    order = np.argsort(-det[:, -1])
    gt_area = (allgt[:, 2] - allgt[:, 0]) * (allgt[:, 3] - allgt[:, 1])
    for k, (lo, hi) in enumerate(ranges):
        covered = np.zeros(len(allgt), bool)
        out_of_range = np.zeros(len(allgt), bool) if lo is None else (gt_area < lo) | (gt_area >= hi)
        for i in order:
            if best[i] >= iou_thr:
                j = arg[i]
                if is_ig[j] or out_of_range[j]:
                    continue
                if covered[j]:
                    fp[k, i] = 1
                else:
                    covered[j], tp[k, i] = True, 1
            elif lo is None or lo <= det_area[i] < hi:
                fp[k, i] = 1
    return tp, fp


def get_cls_results(det_results, annotations, class_id):
    """Per image: the class's detections, ground truth and ignore boxes."""
    dets = [r[class_id] for r in det_results]
    gts, igs = [], []
    for a in annotations:
        gts.append(np.asarray(a['bboxes'])[np.asarray(a['labels']) == class_id, :])
        if a.get('labels_ignore', None) is not None:
            igs.append(np.asarray(a['bboxes_ignore'])[np.asarray(a['labels_ignore']) == class_id, :])
        else:
            igs.append(np.empty((0, 4), dtype=np.float32))
    return dets, gts, igs


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5, dataset=None, logger=None):
    """det_results[img][cls] = (k, 5) xyxy + score; annotations[img] = dict(bboxes, labels[, bboxes_ignore, labels_ignore]).
    scale_ranges: [(lo, hi), ...] in sqrt(area).  dataset='voc07' selects 11-point AP.  Returns (mean_ap, per-class dicts of
    num_gts, num_dets, recall, precision, ap); mean_ap averages the classes with ground truth (per scale: a list)."""
    assert len(det_results) == len(annotations)
    num_classes = len(det_results[0])
    nscale = len(scale_ranges) if scale_ranges is not None else 1
    area_ranges = [(lo ** 2, hi ** 2) for lo, hi in scale_ranges] if scale_ranges is not None else None
    mode = '11points' if dataset == 'voc07' else 'area'
    results = []
    for c in range(num_classes):
        dets, gts, igs = get_cls_results(det_results, annotations, c)
        tpfp = [tpfp_default(d, g, i, iou_thr, area_ranges) for d, g, i in zip(dets, gts, igs)]
        num_gts = np.zeros(nscale, dtype=int)
        for g in gts:
            g = np.asarray(g).reshape(-1, 4)
            if area_ranges is None:
                num_gts[0] += g.shape[0]
            else:
                a = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
                for k, (lo, hi) in enumerate(area_ranges):
                    num_gts[k] += np.sum((a >= lo) & (a < hi))
        dets = np.vstack([np.asarray(d).reshape(-1, 5) for d in dets])
        order = np.argsort(-dets[:, -1])
        results.append(_cls_result(np.hstack([t for t, _ in tpfp]), np.hstack([f for _, f in tpfp]), order, num_gts, mode,
                                   scale_ranges is None))
    return _map_summary(results, scale_ranges, nscale, logger)


def _cls_result(tp, fp, order, num_gts, mode, single):
    """One class of eval_map from its tp / fp flags [num_scales, num_dets], the detections' descending-score `order` and the
    ground-truth counts [num_scales] (the tail of mean_ap.py's per-class loop); shared with eval_map_device."""
    eps = np.finfo(np.float32).eps
    tp = np.cumsum(tp[:, order], axis=1)
    fp = np.cumsum(fp[:, order], axis=1)
    rec = tp / np.maximum(num_gts[:, None], eps)
    prec = tp / np.maximum(tp + fp, eps)
    if single:
        rec, prec, num_gts = rec[0], prec[0], num_gts.item()
    return dict(num_gts=num_gts, num_dets=tp.shape[1], recall=rec, precision=prec, ap=average_precision(rec, prec, mode))


def _map_summary(results, scale_ranges, nscale, logger):
    """The mean over the classes with ground truth and the log lines of eval_map."""
    if scale_ranges is not None:
        aps = np.vstack([r['ap'] for r in results])
        ngt = np.vstack([r['num_gts'] for r in results])
        mean_ap = [aps[ngt[:, k] > 0, k].mean() if np.any(ngt[:, k] > 0) else 0.0 for k in range(nscale)]
    else:
        aps = [r['ap'] for r in results if r['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    if logger is not None and logger != 'silent':
        for c, r in enumerate(results):
            logger.info('class %d: gts %s dets %d ap %s', c, r['num_gts'], r['num_dets'], np.round(r['ap'], 3))
        logger.info('mAP %s', mean_ap)
    return mean_ap, results


def voc_evaluate(results, annotations, metric='mAP', iou_thr=0.5, year=2007, logger=None, device=False, num_classes=None):
    """VOCDataset.evaluate(metric='mAP') (voc.py:27-90): AP<iou*100> per IoU threshold (rounded to 3 places) and their mean as
    'mAP'; VOC 2007 uses the 11-point AP, other years the area.  `device`: match on the GPU (eval_map_device; `results` may then
    be the device triple, with `num_classes`)."""
    if not isinstance(metric, str):
        assert len(metric) == 1
        metric = metric[0]
    if metric != 'mAP':
        raise KeyError(f'metric {metric} is not supported')
    thrs = [iou_thr] if isinstance(iou_thr, float) else list(iou_thr)
    out, means = OrderedDict(), []
    for t in thrs:
        if device:
            m, _ = eval_map_device(results, annotations, iou_thr=t, dataset='voc07' if year == 2007 else None, logger=logger,
                                   num_classes=num_classes)
        else:
            m, _ = eval_map(results, annotations, scale_ranges=None, iou_thr=t, dataset='voc07' if year == 2007 else None,
                            logger=logger)
        means.append(m)
        out[f'AP{int(t * 100):02d}'] = round(m, 3)
    out['mAP'] = sum(means) / len(means)
    return out


def voc_annotations(ds):
    """The per-image VOC annotation dicts of a dataset object: its own (`get_ann_info` / `annotations` in VOC form), or its
    COCO-form `annotations` converted (xywh -> xyxy, category_id -> index in `cat_ids`, iscrowd -> ignore box)."""
    if hasattr(ds, 'get_ann_info'):
        return [ds.get_ann_info(i) for i in range(len(ds))]
    out = []
    for anns in ds.annotations:
        if isinstance(anns, dict):
            out.append(anns)
            continue
        box = {0: [], 1: []}
        lab = {0: [], 1: []}
        for a in anns:
            x, y, w, h = a['bbox']
            crowd = int(bool(a.get('iscrowd', 0)))
            box[crowd].append([x, y, x + w, y + h])
            lab[crowd].append(ds.cat_ids.index(a['category_id']))
        out.append(dict(bboxes=np.array(box[0], np.float32).reshape(-1, 4), labels=np.array(lab[0], np.int64),
                        bboxes_ignore=np.array(box[1], np.float32).reshape(-1, 4), labels_ignore=np.array(lab[1], np.int64)))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Evaluation on the device (csrc/evalmap.hip).  The detections stay where dsl_fcos_detect left them; they are
# packed with torch sorts into (category, image) cells, matched by dsl_eval_match, and - for the COCO protocol - accumulated
# by dsl_eval_accumulate.  Every figure equals the host path's bit for bit; only the closing means run on the host, in the
# host path's own code.
class GtPack:
    """The ground truth of a dataset flattened once (host numpy): boxes [G, 4] float64 (COCO x, y, w, h; VOC x1, y1, x2, y2 of
    float32 values), area [G], crowd / ignore [G] uint8, ordered by (category, image, annotation order - VOC: regular boxes
    before ignore boxes), off [C * NI + 1] int32."""

    def __init__(self, mode, num_cats, num_imgs, key, boxes, area, crowd, ignore):
        key = np.asarray(key, np.int64).reshape(-1)
        order = np.argsort(key, kind='stable')
        self.mode, self.num_cats, self.num_imgs = mode, num_cats, num_imgs
        self.boxes = np.asarray(boxes, np.float64).reshape(-1, 4)[order]
        self.area = np.asarray(area, np.float64).reshape(-1)[order]
        self.crowd = np.asarray(crowd, np.uint8).reshape(-1)[order]
        self.ignore = np.asarray(ignore, np.uint8).reshape(-1)[order]
        cnt = np.bincount(key, minlength=num_cats * num_imgs) if num_cats * num_imgs else np.zeros(0, np.int64)
        self.off = np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)
        self.max_per_cell = int(cnt.max()) if cnt.size else 0
        self._dev = {}

    def to(self, device):
        """The arrays as tensors on `device` (cached: the annotations do not change between evaluations)."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = tuple(torch.from_numpy(a).to(device) for a in (self.boxes, self.area, self.crowd, self.ignore, self.off))
        return self._dev[device]


def flatten_annotations(annotations, img_ids, cat_ids, mode):
    """mode 'coco': annotations[idx] = list of dict(bbox xywh, category_id, iscrowd, [area]); an annotation whose category is
    not in cat_ids is dropped (coco_bbox_eval never looks at it), `area` overrides w * h.  mode 'voc': annotations[idx] =
    dict(bboxes, labels[, bboxes_ignore, labels_ignore]) with 0-based labels; cat_ids = range(num_classes)."""
    NI, C = len(img_ids), len(cat_ids)
    key, box, area, crowd, ign = [], [], [], [], []
    if mode == 'coco':
        index = {c: i for i, c in enumerate(cat_ids)}
        for idx, anns in enumerate(annotations):
            for a in anns:
                ci = index.get(a['category_id'])
                if ci is None:
                    continue
                key.append(ci * NI + idx)
                box.append([float(v) for v in a['bbox'][:4]])
                area.append(a.get('area', a['bbox'][2] * a['bbox'][3]))
                crowd.append(bool(a.get('iscrowd', 0)))
                ign.append(0)
    elif mode == 'voc':
        for flag, kb, kl in ((0, 'bboxes', 'labels'), (1, 'bboxes_ignore', 'labels_ignore')):       # all regular boxes first: the stable
            for idx, a in enumerate(annotations):                                                   # sort keeps them ahead in each cell
                if a.get(kl, None) is None:
                    continue
                lab = np.asarray(a[kl]).reshape(-1)
                b = np.asarray(a[kb], np.float32).reshape(-1, 4)
                for j in np.nonzero((lab >= 0) & (lab < C))[0]:
                    key.append(int(lab[j]) * NI + idx)
                    box.append(b[j].astype(np.float64))
                    area.append(0.0)
                    crowd.append(0)
                    ign.append(flag)
    else:
        raise ValueError(f"mode {mode!r}: 'coco' or 'voc'")
    return GtPack(mode, C, NI, key, box, area, crowd, ign)


class EvalPack:
    """pack_eval_inputs' result: the arrays dsl_eval_match / dsl_eval_accumulate read, on the detections' device."""


def pack_eval_inputs(dets, labels, count, annotations, img_ids, cat_ids, mode, max_dets=100):
    """Pure torch (CPU tensors too).  dets [N, K, 5] xyxy + score, labels [N, K] class indices, count [N] valid rows per image;
    annotations: the per-image lists / dicts, or a GtPack made by flatten_annotations.  The valid rows are sorted stably by
    descending score, then stably by cell = label * NI + image, so that a cell holds its rows by rank (ties in array order,
    det2json's order); rows of rank >= max_dets are cut (None: no cut).  Returns an EvalPack:
      det_boxes [M, 4] float32, det_scores [M], det_src [M] (row n * K + k of the input), det_off [C * NI + 1] int32,
      perm [M] int32: per category the rows by descending score, ties by (image, rank);
      gt_boxes / gt_area / gt_crowd / gt_ignore / gt_off, max_gt_per_cell, num_cats, num_imgs, mode."""
    gt = annotations if isinstance(annotations, GtPack) else flatten_annotations(annotations, img_ids, cat_ids, mode)
    NI, C = len(img_ids), len(cat_ids)
    assert (gt.mode, gt.num_cats, gt.num_imgs) == (mode, C, NI), 'the flattened annotations belong to another dataset or protocol'
    N, K = labels.shape
    assert N == NI, f'The length of results is not equal to the dataset len: {N} != {NI}'
    dev = dets.device
    valid = (torch.arange(K, device=dev)[None] < count.to(torch.int64)[:, None]) & (labels >= 0) & (labels < C)
    src = valid.reshape(-1).nonzero().reshape(-1)                  # (image, slot) order = array order
    flat = dets.reshape(N * K, 5)[src].to(torch.float32)
    score, lab, img = flat[:, 4], labels.reshape(-1)[src].to(torch.int64), src // max(K, 1)
    o1 = torch.sort(-score, stable=True).indices
    key = (lab * NI + img)[o1]
    key, o2 = torch.sort(key, stable=True)
    order = o1[o2]
    ncell = C * NI
    cnt = torch.bincount(key, minlength=ncell)
    if max_dets is not None and key.numel():
        rank = torch.arange(key.numel(), device=dev) - (torch.cumsum(cnt, 0) - cnt)[key]
        keep = rank < max_dets
        order, key = order[keep], key[keep]
        cnt = torch.bincount(key, minlength=ncell)
    p = EvalPack()
    p.mode, p.num_cats, p.num_imgs, p.max_gt_per_cell = mode, C, NI, gt.max_per_cell
    p.det_boxes, p.det_scores, p.det_src = flat[order, :4].contiguous(), score[order].contiguous(), src[order]
    p.det_off = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0))).to(torch.int32)
    q1 = torch.sort(-p.det_scores, stable=True).indices
    q2 = torch.sort(torch.div(key, max(NI, 1), rounding_mode='floor')[q1], stable=True).indices
    p.perm = q1[q2].to(torch.int32)
    p.gt_boxes, p.gt_area, p.gt_crowd, p.gt_ignore, p.gt_off = gt.to(dev)
    return p


def _as_triple(results, device=None):
    """The device triple as it is, or reference-format results[img][label] = (k, 5) arrays uploaded as one (rows of an image in
    (label, array) order - det2json's)."""
    if isinstance(results, tuple) and len(results) == 3 and all(isinstance(t, torch.Tensor) for t in results):
        return results
    device = device or 'cuda'
    N = len(results)
    per = [[np.asarray(b, np.float32).reshape(-1, 5) for b in r] for r in results]
    cnt = np.array([sum(len(b) for b in r) for r in per], np.int32).reshape(N)
    K = max(int(cnt.max()) if N else 0, 1)
    dets, labels = np.zeros((N, K, 5), np.float32), np.zeros((N, K), np.int64)
    for i, r in enumerate(per):
        if cnt[i]:
            dets[i, :cnt[i]] = np.concatenate(r)
            labels[i, :cnt[i]] = np.concatenate([np.full(len(b), c, np.int64) for c, b in enumerate(r)])
    return torch.from_numpy(dets).to(device), torch.from_numpy(labels).to(device), torch.from_numpy(cnt).to(device)


def triple_to_results(triple, num_classes):
    """(dets, labels, count) -> the reference format, as sweep.simple_test builds it."""
    from .sweep import bbox2result
    dets, labels, count = (t.cpu().numpy() for t in triple)
    return [bbox2result(dets[i, :count[i]], labels[i, :count[i]], num_classes) for i in range(len(count))]


def coco_bbox_eval_device(results, img_ids, cat_ids, annotations, iou_thrs=None, max_dets=100, return_precision=False, device=None):
    """coco_bbox_eval on the GPU.  `results`: the device triple (dets [N, K, 5], labels [N, K], count [N]) or the reference
    format results[img][label] = (k, 5), which is uploaded; `annotations` as coco_bbox_eval's, or a GtPack.  Returns what
    coco_bbox_eval returns for det2json(results), bit for bit (the same `return_precision` form)."""
    from . import _lib as L
    from . import ops
    iou_thrs = np.linspace(.5, .95, 10) if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    dets, labels, count = _as_triple(results, device)
    p = pack_eval_inputs(dets, labels, count, annotations, img_ids, cat_ids, 'coco', max_dets)
    dev = dets.device
    thr = torch.from_numpy(np.ascontiguousarray(iou_thrs, np.float64)).to(dev)
    rng = torch.tensor([[float(lo), float(hi)] for lo, hi in COCO_AREA_RANGES.values()], dtype=torch.float64, device=dev)
    rec = torch.from_numpy(np.linspace(0, 1, 101)).to(dev)
    matched, ignored, npos = ops.eval_match(L.EVAL_COCO, p.num_cats, p.num_imgs, p.det_boxes, p.det_off, p.gt_boxes, p.gt_area,
                                            p.gt_crowd, p.gt_ignore, p.gt_off, p.max_gt_per_cell, thr, rng)
    table = ops.eval_accumulate(p.num_cats, p.num_imgs, matched, ignored, npos, p.det_off, p.perm, rec).cpu().numpy()
    prec = {r: table[i] for i, r in enumerate(COCO_AREA_RANGES)}
    metrics = _coco_summary(prec, iou_thrs)
    return (metrics, prec) if return_precision else metrics


def _f32_threshold(t):
    """tpfp_default compares a float32 IoU with `iou_thr` under numpy's promotion rules: a Python float is weak (the comparison
    runs in float32, i.e. against float32(t)), a numpy float64 is not.  The kernel compares in fp64 against this value."""
    return float(np.float32(t)) if (np.float32(0) + t).dtype == np.float32 else float(t)


def voc_match_device(p, iou_thr=0.5):
    """dsl_eval_match(DSL_EVAL_VOC) over an EvalPack: (tp, fp) uint8 [M] on the device, in the pack's row order."""
    from . import _lib as L
    from . import ops
    dev = p.det_boxes.device
    thr = torch.tensor([_f32_threshold(iou_thr)], dtype=torch.float64, device=dev)
    rng = torch.tensor([[0.0, 1e10]], dtype=torch.float64, device=dev)
    tp, fp, _ = ops.eval_match(L.EVAL_VOC, p.num_cats, p.num_imgs, p.det_boxes, p.det_off, p.gt_boxes, p.gt_area, p.gt_crowd,
                               p.gt_ignore, p.gt_off, p.max_gt_per_cell, thr, rng)
    return tp, fp


def eval_map_device(results, annotations, iou_thr=0.5, dataset=None, logger=None, num_classes=None, device=None):
    """eval_map(scale_ranges=None) with tpfp_default's flags computed on the GPU; the per-class ordering, cumsum and
    average_precision are eval_map's own code, over the class's rows put back into eval_map's row order (image, array order).
    `results`: the device triple (then `num_classes` is required) or results[img][cls] = (k, 5).
    One difference: tpfp_default visits the detections of an (image, class) cell by np.argsort(-score), which is not a stable
    sort, so parity of the flags is defined for distinct scores within a cell; the kernel visits equal scores in array order
    (the rank of pack_eval_inputs)."""
    if num_classes is None:
        num_classes = len(results[0]) if not isinstance(results, tuple) else None
    assert num_classes is not None, 'eval_map_device: num_classes is required with the device triple'
    dets, labels, count = _as_triple(results, device)
    N = labels.shape[0]
    gt = annotations if isinstance(annotations, GtPack) else flatten_annotations(annotations, range(N), range(num_classes), 'voc')
    assert N == gt.num_imgs
    p = pack_eval_inputs(dets, labels, count, gt, range(N), range(num_classes), 'voc', max_dets=None)
    tp, fp = voc_match_device(p, iou_thr)
    tp, fp = tp.cpu().numpy().astype(np.float32), fp.cpu().numpy().astype(np.float32)
    off, src, score = p.det_off.cpu().numpy(), p.det_src.cpu().numpy(), p.det_scores.cpu().numpy()
    mode = '11points' if dataset == 'voc07' else 'area'
    results = []
    for c in range(num_classes):
        s0, s1 = int(off[c * N]), int(off[(c + 1) * N])
        g0, g1 = int(gt.off[c * N]), int(gt.off[(c + 1) * N])
        num_gts = np.array([int((gt.ignore[g0:g1] == 0).sum())], dtype=int)
        back = s0 + np.argsort(src[s0:s1], kind='stable')          # (category, image, rank) -> eval_map's (image, array order)
        results.append(_cls_result(tp[None, back], fp[None, back], np.argsort(-score[back]), num_gts, mode, True))
    return _map_summary(results, None, 1, logger)


class VOCEvalDataset:
    """The evaluation side of VOCDataset as a plain object: `annotations` one dict per image (bboxes, labels, bboxes_ignore,
    labels_ignore), `year` 2007 (11-point AP) or 2012 (area); `evaluate` is voc.py's."""

    def __init__(self, annotations, year=2007, CLASSES=None):
        self.annotations, self.year, self.CLASSES = list(annotations), year, CLASSES

    def __len__(self):
        return len(self.annotations)

    def get_ann_info(self, idx):
        return self.annotations[idx]

    def evaluate(self, results, metric='mAP', logger=None, iou_thr=0.5, scale_ranges=None, **kw):
        return voc_evaluate(results, self.annotations, metric=metric, iou_thr=iou_thr, year=self.year, logger=logger)


# ----------------------------------------------------------------------------------------------------------------------
def _unwrap(x):
    return x[0] if isinstance(x, (list, tuple)) and len(x) == 1 and isinstance(x[0], (list, tuple, torch.Tensor)) else x


@torch.no_grad()
def single_gpu_test(model, data_loader, store=None, keep_on_device=False):
    """mmdet/apis/test.py single_gpu_test without the visualisation: per image the list of per-class (k, 5) arrays.
    `keep_on_device`: no host copy per batch - the stacked triple (dets [N, K, 5], labels [N, K], count [N]) of
    sweep.detect_device (of sweep.aug_test_device where the loader yields several views per image) on the GPU."""
    det = model.module if hasattr(model, 'module') else model
    if keep_on_device:
        from .sweep import aug_test_device, detect_device
        dev, parts = det.store.device, []
        for data in data_loader:
            imgs, metas = data['img'], data['img_metas']
            if isinstance(imgs, (list, tuple)) and len(imgs) > 1:          # MultiScaleFlipAug's views of one image
                out = aug_test_device(det, [i.to(dev) for i in imgs], metas, rescale=True, store=store)
            else:
                out = detect_device(det, _unwrap(imgs).to(dev), _unwrap(metas), True, store)
            parts.append(tuple(t.clone() for t in out))
        if not parts:
            return (torch.zeros(0, 1, 5, device=dev), torch.zeros(0, 1, dtype=torch.int64, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev))
        dets, labels, count = (torch.cat([p[k] for p in parts]) for k in range(3))
        if bool((count < 0).any()):
            raise RuntimeError('dsl_fcos_detect_finish: a view of the pool was not collected for an image (det_count = -1)')
        return dets, labels, count
    results = []
    for data in data_loader:
        img, metas = _unwrap(data['img']), _unwrap(data['img_metas'])
        from .sweep import simple_test
        results.extend(simple_test(det, img.to(det.store.device), metas, rescale=True, store=store))
    return results


@torch.no_grad()
def multi_gpu_test(model, data_loader, store=None):
    """Every rank tests its loader's shard (the loader yields rank-local batches, index = rank + k * world as a
    DistributedSampler(shuffle=False) does); results are gathered in dataset order on every rank."""
    import torch.distributed as dist
    part = single_gpu_test(model, data_loader, store)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return part
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, part)
    out = []
    for i in range(max(len(p) for p in parts)):
        out += [p[i] for p in parts if i < len(p)]
    n = getattr(getattr(data_loader, 'dataset', data_loader), 'num_images', len(out))
    return out[:n]


class EvalHook:
    """eval_hooks.py:9-66 on top of mmcv's EvalHook: every `interval` epochs (from `start`), test `dataloader` with the EMA
    teacher if the runner has one (`runner.ema_flag`), else the student; evaluate with the dataset's own `evaluate()` or, for
    datasets that carry `annotations`, the built-in COCO bbox protocol; log the metrics; optionally keep the best checkpoint."""
    priority = 75

    def __init__(self, dataloader, start=None, interval=1, by_epoch=True, save_best=None, metric='bbox', jsonfile_prefix=None,
                 device_eval=False, **eval_kwargs):
        self.dataloader, self.start, self.interval, self.by_epoch = dataloader, start, interval, by_epoch
        # device_eval: 'bbox' / 'mAP' of a dataset without its own evaluate() are matched and accumulated on the GPU
        # (coco_bbox_eval_device / eval_map_device): the same metrics bit for bit, json only for an explicit jsonfile_prefix
        self.device_eval = bool(device_eval)
        self.save_best = 'mAP' if save_best == 'auto' else save_best
        self.metric, self.jsonfile_prefix, self.eval_kwargs = metric, jsonfile_prefix, eval_kwargs
        self.best, self.history = None, []

    def __getattr__(self, name):
        if name.startswith(('before_', 'after_')):
            return lambda runner: None
        raise AttributeError(name)

    def _should_evaluate(self, runner):
        cur = runner.epoch + 1
        if self.start is not None and cur < self.start:
            return False
        return (cur - (self.start or 0)) % self.interval == 0 if self.start is not None else cur % self.interval == 0

    def after_train_epoch(self, runner):
        if self.by_epoch and self._should_evaluate(runner):
            self._do_evaluate(runner)

    @staticmethod
    def _gt_pack(ds, mode, make):
        """The dataset's flattened ground truth, made once and kept on the dataset object."""
        cache = getattr(ds, '_device_eval_gt', None)
        if cache is None:
            cache = {}
            try:
                ds._device_eval_gt = cache
            except AttributeError:
                pass
        if mode not in cache:
            cache[mode] = make()
        return cache[mode]

    def _device_metrics(self, ds, results, num_classes):
        if self.metric in ('mAP', ['mAP']):
            n = results[2].numel() if isinstance(results, tuple) else len(results)
            gt = self._gt_pack(ds, 'voc', lambda: flatten_annotations(voc_annotations(ds), range(n), range(num_classes), 'voc'))
            return voc_evaluate(results, gt, year=getattr(ds, 'year', 2007), device=True, num_classes=num_classes, **self.eval_kwargs)
        gt = self._gt_pack(ds, 'coco', lambda: flatten_annotations(ds.annotations, ds.img_ids, ds.cat_ids, 'coco'))
        if self.jsonfile_prefix:
            host = triple_to_results(results, num_classes) if isinstance(results, tuple) else results
            format_results(host, ds.img_ids, ds.cat_ids, self.jsonfile_prefix)
        metrics = coco_bbox_eval_device(results, ds.img_ids, ds.cat_ids, gt)
        return OrderedDict((f'bbox_{k}', v) for k, v in metrics.items())

    def _do_evaluate(self, runner):
        det = runner._det(runner.model)
        store = runner._det(runner.ema_model).store if (runner.ema_flag and runner.ema_model is not None) else None
        if store is not None and runner.logger:
            runner.logger.info('Using ema model for eval')
        import torch.distributed as dist
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        ds = getattr(self.dataloader, 'dataset', self.dataloader)
        on_device = self.device_eval and not hasattr(ds, 'evaluate') and self.metric in ('bbox', ['bbox'], 'mAP', ['mAP'])
        if on_device and not multi:
            results = single_gpu_test(det, self.dataloader, store, keep_on_device=True)      # the triple goes straight in
        else:
            results = multi_gpu_test(det, self.dataloader, store)      # several ranks: the object gather, then the list form
        # DistEvalHook (mmdet/core/evaluation/eval_hooks.py): every rank takes part in the gather above, but only rank 0 formats,
        # evaluates, logs and saves - the other ranks would race on the same json / checkpoint paths - and the metrics are
        # broadcast so every rank's history / best agree
        rank = dist.get_rank() if multi else 0
        metrics = None
        if rank == 0:
            if hasattr(ds, 'evaluate'):
                metrics = ds.evaluate(results, metric=self.metric, **self.eval_kwargs)
            elif on_device:
                metrics = self._device_metrics(ds, results, det.bbox_head.num_classes)
            elif self.metric in ('mAP', ['mAP']):
                metrics = voc_evaluate(results, voc_annotations(ds), year=getattr(ds, 'year', 2007), **self.eval_kwargs)
            else:
                prefix = self.jsonfile_prefix or (os.path.join(runner.work_dir, f'eval_epoch_{runner.epoch + 1}') if runner.work_dir else None)
                files, tmp = format_results(results, ds.img_ids, ds.cat_ids, prefix)
                metrics = coco_bbox_eval(json.load(open(files['bbox'])), ds.img_ids, ds.cat_ids, ds.annotations)
                metrics = OrderedDict((f'bbox_{k}', v) for k, v in metrics.items())
                if tmp is not None:
                    tmp.cleanup()
        if multi:
            box = [metrics]
            dist.broadcast_object_list(box, src=0)
            metrics = box[0]
        self.history.append((runner.epoch + 1, dict(metrics)))
        if runner.logger and rank == 0:
            runner.logger.info('Epoch(val) [%d]\t%s', runner.epoch + 1, ', '.join(f'{k}: {v:.4f}' for k, v in metrics.items()))
        key = next((k for k in metrics if self.save_best and k.endswith(self.save_best)), None)
        if key is not None and (self.best is None or metrics[key] > self.best) and runner.work_dir:
            self.best = metrics[key]
            if rank == 0:
                runner.save_checkpoint(runner.work_dir, filename_tmpl='best_' + key + '_epoch_{}.pth', create_symlink=False)
        if multi:
            dist.barrier()
        return metrics


def load_checkpoint(model, filename, map_location='cpu', strict=False, revise_keys=((r'^module\.', ''),)):
    """mmcv.runner.load_checkpoint for upstream .pth files: optional 'state_dict' wrapper, key rewriting
    (default: strip DDP's 'module.'), non-strict by default.  Returns the checkpoint dict."""
    import re
    ck = torch.load(filename, map_location=map_location)
    sd = ck.get('state_dict', ck) if isinstance(ck, dict) else ck
    for pat, rep in revise_keys:
        sd = OrderedDict((re.sub(pat, rep, k), v) for k, v in sd.items())
    det = model.module if hasattr(model, 'module') else model
    det.load_state_dict(sd, strict=strict)
    return ck
