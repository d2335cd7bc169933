"""Time one COCO bbox evaluation on the host path (format_results + json.load + coco_bbox_eval, as EvalHook runs it by default)
and on the device path (pack_eval_inputs + dsl_eval_match + dsl_eval_accumulate + the copy of the precision table + the means),
on one synthetic set from one generator.  A report, not a gate (DESIGN.md section 3.4b holds the figures).

  python tools/bench_eval.py [--images 5000] [--categories 80] [--dets 42 100] [--repeats 5] [--no-host]

Per --dets value one JSON line: host seconds (one run: it takes minutes at full size), device seconds (median of --repeats after
a warm-up run, synchronised before each clock read), the per-stage medians, and whether the two paths returned the same metrics."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = np.array([(32., 32.), (96., 96.), (16., 64.), (48., 192.), (20., 20.), (50., 50.), (150., 120.), (31.5, 32.5), (96., 96.25)])


def generate(n_images, n_cats, dets_per_img, seed=0):
    """Per image ~7 ground-truth boxes whose areas straddle and sit on 32^2 / 96^2 (30 % with an explicit `area`, 5 % crowd) and
    `dets_per_img` detections: jittered copies of ground truth (85 % with its category) and false positives, scores in 1/8 steps.
    Returns (results[img][label] = (k, 5) float32, img_ids, cat_ids, annotations)."""
    rng = np.random.RandomState(seed)
    img_ids, cat_ids = list(range(1, n_images + 1)), list(range(1, n_cats + 1))
    results, anns = [], []
    for _ in range(n_images):
        g = int(np.clip(rng.poisson(7), 1, 40))
        wh = SIZES[rng.randint(len(SIZES), size=g)] * np.where(rng.rand(g, 1) < .4, rng.uniform(.7, 1.3, (g, 2)), 1.)
        xy = np.stack((rng.uniform(0, 400, g), rng.uniform(0, 300, g)), 1)
        cat = rng.randint(n_cats, size=g)
        a = []
        for k in range(g):
            d = dict(bbox=[float(xy[k, 0]), float(xy[k, 1]), float(wh[k, 0]), float(wh[k, 1])], category_id=cat_ids[cat[k]],
                     iscrowd=int(rng.rand() < .05))
            if rng.rand() < .3:
                d['area'] = float(rng.choice([1024., 9216., wh[k, 0] * wh[k, 1] * .8, 500.]))
            a.append(d)
        anns.append(a)
        n_hit = int(dets_per_img * .6)
        src = rng.randint(g, size=n_hit)
        box = np.hstack((xy[src], wh[src])) + rng.normal(0, .1, (n_hit, 4)) * np.tile(wh[src], 2) * (rng.rand(n_hit, 1) < .8)
        box[:, 2:] = np.maximum(box[:, 2:], 2.)
        lab = np.where(rng.rand(n_hit) < .85, cat[src], rng.randint(n_cats, size=n_hit))
        n_fp = dets_per_img - n_hit
        box = np.vstack((box, np.stack((rng.uniform(0, 400, n_fp), rng.uniform(0, 300, n_fp), np.full(n_fp, 30.), np.full(n_fp, 30.)), 1)))
        lab = np.concatenate((lab, rng.randint(n_cats, size=n_fp)))
        score = rng.randint(1, 9, size=dets_per_img) / 8.
        rows = np.hstack((box[:, :2], box[:, :2] + box[:, 2:], score[:, None])).astype(np.float32)
        results.append([rows[lab == c] for c in range(n_cats)])
    return results, img_ids, cat_ids, anns


def host_path(E, results, img_ids, cat_ids, anns):
    t0 = time.perf_counter()
    files, tmp = E.format_results(results, img_ids, cat_ids)
    with open(files['bbox']) as f:
        dets = json.load(f)
    t1 = time.perf_counter()
    m = E.coco_bbox_eval(dets, img_ids, cat_ids, anns)
    t2 = time.perf_counter()
    tmp.cleanup()
    return m, dict(json=t1 - t0, coco_bbox_eval=t2 - t1, total=t2 - t0)


def device_path(E, triple, img_ids, cat_ids, gt):
    """coco_bbox_eval_device stage by stage (the same calls), with a synchronise before each clock read."""
    from dsl_amd import _lib as L
    from dsl_amd import ops
    dev = triple[0].device

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()
    iou_thrs = np.linspace(.5, .95, 10)
    t0 = clock()
    p = E.pack_eval_inputs(*triple, gt, img_ids, cat_ids, 'coco', 100)
    thr = torch.from_numpy(iou_thrs).to(dev)
    rng = torch.tensor([[float(lo), float(hi)] for lo, hi in E.COCO_AREA_RANGES.values()], dtype=torch.float64, device=dev)
    rec = torch.from_numpy(np.linspace(0, 1, 101)).to(dev)
    t1 = clock()
    matched, ignored, npos = ops.eval_match(L.EVAL_COCO, p.num_cats, p.num_imgs, p.det_boxes, p.det_off, p.gt_boxes, p.gt_area, p.gt_crowd,
                                            p.gt_ignore, p.gt_off, p.max_gt_per_cell, thr, rng)
    t2 = clock()
    table = ops.eval_accumulate(p.num_cats, p.num_imgs, matched, ignored, npos, p.det_off, p.perm, rec)
    t3 = clock()
    table = table.cpu().numpy()
    m = E._coco_summary({r: table[i] for i, r in enumerate(E.COCO_AREA_RANGES)}, iou_thrs)
    t4 = clock()
    return m, dict(pack=t1 - t0, match=t2 - t1, accumulate=t3 - t2, copy_and_means=t4 - t3, total=t4 - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--categories', type=int, default=80)
    ap.add_argument('--dets', type=int, nargs='+', default=[42, 100])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    from dsl_amd import evaluation as E
    for D in args.dets:
        results, img_ids, cat_ids, anns = generate(args.images, args.categories, D)
        t0 = time.perf_counter()
        gt = E.flatten_annotations(anns, img_ids, cat_ids, 'coco')
        flatten = time.perf_counter() - t0
        triple = E._as_triple(results, 'cuda')
        device_path(E, triple, img_ids, cat_ids, gt)                       # warm-up
        runs = [device_path(E, triple, img_ids, cat_ids, gt) for _ in range(args.repeats)]
        dev = {k: statistics.median(r[1][k] for r in runs) for k in runs[0][1]}
        out = dict(images=args.images, categories=args.categories, dets_per_img=D, detections=int(triple[2].sum()),
                   device_s={k: round(v, 6) for k, v in dev.items()}, flatten_annotations_once_s=round(flatten, 4))
        if not args.no_host:
            hm, host = host_path(E, results, img_ids, cat_ids, anns)
            out.update(host_s={k: round(v, 3) for k, v in host.items()}, speedup=round(host['total'] / dev['total'], 1),
                       same_metrics=list(hm.items()) == list(runs[-1][0].items()))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
