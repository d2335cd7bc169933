"""Generate the class-count fixtures (tests/golden/loss_c{1,3,20}.npz, voc_map.npz) by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_golden_classes.py
  loss_c<C>.npz  FCOSHead.loss of a C-class head (same recipe as make_golden.gen_loss's 'loss_dsl': B = 3, sisoft on, ignore
                 boxes, image 2 = image 1 at half size)
  voc_map.npz    eval_map (mmdet/core/evaluation/mean_ap.py, its functions taken out of the file with `ast` and run
                 in-process: no multiprocessing pool, no table printing) on synthetic detections / ground truth of 20 classes
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, O, SUP_CFG, save  # noqa: E402

CLASS_COUNTS = (1, 3, 20)
VOC_C = 20
VOC_CASES = (('11points', None, 0.5), ('11points', None, 0.75), ('area', None, 0.5), ('area', None, 0.75),
             ('area', ((0, 32), (32, 96), (96, 1e5)), 0.5), ('11points', ((0, 32), (32, 96), (96, 1e5)), 0.5))


def gts_for(rng, H, W, n, C, lo=8.0, hi=None):
    b = O.synth_boxes(rng, n, H=H, W=W, lo=lo, hi=hi or max(H, W))
    return torch.from_numpy(b), torch.from_numpy(rng.randint(0, C, len(b)).astype('int64'))


def gen_loss_classes():
    sizes = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]       # 128 x 192 canvas
    B, lw, sw = 3, 3.0, 1.0
    for C in CLASS_COUNTS:
        head = R.build_fcos(SUP_CFG, num_classes=C).bbox_head
        rng = np.random.RandomState(100 + C)
        g = torch.Generator().manual_seed(1000 + C)
        cls = [(torch.randn(B, C, h, w, generator=g) * 1.5 - 2.0).requires_grad_() for h, w in sizes]
        reg = [(torch.rand(B, 4, h, w, generator=g) * 6.0 * (torch.rand(B, 4, h, w, generator=g) > 0.1)).requires_grad_()
               for h, w in sizes]
        ctr = [torch.randn(B, 1, h, w, generator=g).requires_grad_() for h, w in sizes]
        gtb, gtl, igb = [], [], []
        for i in range(B):
            b, l = gts_for(rng, 128, 192, int(rng.randint(1, 6)), C, lo=8.0, hi=160.0)
            ib, _ = gts_for(rng, 128, 192, int(rng.randint(0, 4)), C, lo=8.0, hi=100.0)
            gtb.append(b)
            gtl.append(l)
            igb.append(ib)
        gtb[2], gtl[2], igb[2] = gtb[1] / 2, gtl[1], igb[1] / 2
        head.loss_weight, head.soft_weight, head.soft_warm_up, head.cur_iter = lw, sw, 0, 0
        losses = head.loss(cls, reg, ctr, gtb, gtl, [dict(img_shape=(128, 192, 3))] * B, gt_bboxes_ignore=igb)
        sum(v for v in losses.values()).backward()
        d = dict(sizes=np.array(sizes), B=B, num_classes=C, loss_weight=lw, soft_weight=sw, soft_warm_up=0, with_ig=1)
        for i in range(B):
            d[f'gt{i}'], d[f'gl{i}'], d[f'ig{i}'] = gtb[i], gtl[i], igb[i]
        for i in range(5):
            d[f'cls{i}'], d[f'reg{i}'], d[f'ctr{i}'] = cls[i], reg[i], ctr[i]
            d[f'gcls{i}'], d[f'greg{i}'], d[f'gctr{i}'] = cls[i].grad, reg[i].grad, ctr[i].grad
        for k, v in losses.items():
            d[k] = np.float64(float(v))
        save(f'loss_c{C}.npz', **d)


def _mean_ap_namespace():
    ev = os.path.join(R.REF, 'mmdet/core/evaluation')
    ns = dict(np=np)
    src = open(os.path.join(ev, 'bbox_overlaps.py')).read()
    exec(compile(src, os.path.join(ev, 'bbox_overlaps.py'), 'exec'), ns)
    path = os.path.join(ev, 'mean_ap.py')
    want = ('average_precision', 'tpfp_default', 'get_cls_results', 'eval_map')
    fns = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == len(want)

    class InProcessPool:                  # eval_map's Pool(nproc): the same starmap, in this process
        def __init__(self, *a, **k):
            pass

        def starmap(self, fn, it):
            return [fn(*args) for args in it]

        def close(self):
            pass

    ns.update(Pool=InProcessPool, print_map_summary=lambda *a, **k: None)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, 'exec'), ns)
    return ns


def _voc_case(rng, n_img=40):
    """Detections around jittered ground truth plus background false positives; classes 5 and 12 have detections but no
    ground truth, class 17 neither; ignore boxes on about a third of the images; a few duplicate detections and tied scores."""
    dets, anns = [], []
    for _ in range(n_img):
        n = int(rng.randint(0, 9))
        b = O.synth_boxes(rng, n, H=500, W=500, lo=6.0, hi=300.0).astype(np.float32).reshape(-1, 4)
        lab = rng.choice([c for c in range(VOC_C) if c not in (5, 12, 17)], size=len(b)).astype(np.int64)
        k = int(rng.randint(0, 3)) if rng.rand() < 0.35 else 0
        ib = O.synth_boxes(rng, k, H=500, W=500, lo=6.0, hi=200.0).astype(np.float32).reshape(-1, 4)
        il = rng.randint(0, VOC_C, len(ib)).astype(np.int64)
        anns.append(dict(bboxes=b, labels=lab, bboxes_ignore=ib, labels_ignore=il))
        per = [[] for _ in range(VOC_C)]
        for box, l in zip(np.vstack([b, ib]), np.concatenate([lab, il])):
            for _ in range(int(rng.randint(0, 3))):
                wh = np.array([box[2] - box[0], box[3] - box[1]] * 2, np.float32)
                jit = box + rng.randn(4).astype(np.float32) * 0.12 * wh
                c = l if rng.rand() < 0.85 else int(rng.randint(0, VOC_C))
                per[c].append(np.append(jit, np.float32(np.round(rng.rand(), 2))))
        for _ in range(int(rng.randint(0, 5))):
            fb = O.synth_boxes(rng, 1, H=500, W=500, lo=6.0, hi=250.0).astype(np.float32).reshape(4)
            per[int(rng.randint(0, VOC_C))].append(np.append(fb, np.float32(rng.rand() * 0.6)))
        dets.append([np.array(p, np.float32).reshape(-1, 5) for p in per])
    return dets, anns


def gen_voc_map():
    ns = _mean_ap_namespace()
    rng = np.random.RandomState(20)
    dets, anns = _voc_case(rng)
    d = dict(n_img=len(dets), num_classes=VOC_C, n_cases=len(VOC_CASES))
    for i, (det, a) in enumerate(zip(dets, anns)):
        for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore'):
            d[f'ann{i}_{k}'] = a[k]
        for c in range(VOC_C):
            d[f'det{i}_{c}'] = det[c]
    for j, (mode, ranges, iou) in enumerate(VOC_CASES):
        mean_ap, res = ns['eval_map'](dets, anns, scale_ranges=list(ranges) if ranges else None, iou_thr=iou,
                                      dataset='voc07' if mode == '11points' else None, nproc=1)
        d[f'case{j}_mode'] = mode
        d[f'case{j}_iou'] = iou
        d[f'case{j}_ranges'] = np.array(ranges if ranges else np.zeros((0, 2)), np.float64)
        d[f'case{j}_mAP'] = np.array(mean_ap, np.float64)
        d[f'case{j}_ap'] = np.array([r['ap'] for r in res], np.float64)
        d[f'case{j}_num_gts'] = np.array([r['num_gts'] for r in res], np.int64)
        for c, r in enumerate(res):
            d[f'case{j}_rec{c}'] = np.asarray(r['recall'], np.float64)
            d[f'case{j}_prec{c}'] = np.asarray(r['precision'], np.float64)
        print(f'case {j} {mode} ranges={ranges} iou={iou}: mAP {mean_ap}')
    save('voc_map.npz', **d)


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_voc_map()
    gen_loss_classes()
