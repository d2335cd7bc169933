"""Generate the loss-family fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_golden_loss_family.py
  loss_fam_<leg>.npz     FCOSHead.loss of the reference with its loss_cls / loss_bbox / loss_centerness dicts overridden: DIoULoss,
                         CIoULoss, IoULoss(linear=True), FocalLoss gamma / alpha, the three loss_weights - on the 128 x 192 canvas and
                         the head outputs of make_golden_head_options (whose range keeps the reference finite)
The layout is loss_opt_*.npz's (raw `reg`, `scales`, `cls`, `ctr`, boxes, the reference's losses and gradients, the five head
options) plus the loss settings: box_loss (giou / iou / iou_linear / diou / ciou), box_eps, focal_gamma, focal_alpha, cls_weight,
bbox_weight, ctr_weight.  Every leg holds at least MIN_POS positive locations and only finite reference outputs (asserted here).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, SUP_CFG, gts_for, save  # noqa: E402
from make_golden_head_options import MIN_POS, SIZES, TRICKS, head_outputs  # noqa: E402

FOCAL = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
CTR = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)
BOX_TYPES = dict(giou='GIoULoss', iou='IoULoss', iou_linear='IoULoss', diou='DIoULoss', ciou='CIoULoss')
# name -> (head option flips, classes, B, stream loss_weight, soft_weight, box_loss, loss_bbox weight, focal overrides, centerness weight)
LEGS = [
    ('loss_fam_diou', {}, 80, 2, 1.0, 0.0, 'diou', 2.0, {}, 1.0),
    ('loss_fam_ciou', dict(norm_on_bbox=0), 80, 2, 1.0, 0.0, 'ciou', 0.5, {}, 1.0),
    ('loss_fam_ciou_dsl_c18', dict(centerness_on_reg=0), 18, 3, 3.0, 1.0, 'ciou', 1.0, {}, 1.0),
    ('loss_fam_iou_linear', dict(norm_on_bbox=0, center_sampling=0), 80, 2, 1.0, 0.0, 'iou_linear', 1.0, {}, 1.0),
    ('loss_fam_focal_all', {}, 80, 2, 1.0, 0.0, 'giou', 1.5, dict(gamma=1.5, alpha=0.5, loss_weight=0.25), 2.0),
    ('loss_fam_focal_g0', {}, 80, 2, 1.0, 0.0, 'giou', 1.0, dict(gamma=0.0, alpha=0.75), 1.0),
    ('loss_fam_focal_g3', {}, 80, 2, 1.0, 0.0, 'giou', 1.0, dict(gamma=3.0), 1.0),
]


def gen():
    for name, flips, C, B, lw, sw, box, wb, focal, wc in LEGS:
        o = dict(TRICKS, **flips)
        o['iou_loss'] = int(box in ('iou', 'iou_linear'))
        loss_bbox = dict(type=BOX_TYPES[box], loss_weight=wb)
        if box == 'iou_linear':
            loss_bbox['linear'] = True
        loss_cls = dict(FOCAL, **focal)
        head = R.build_fcos(SUP_CFG, num_classes=C, center_sampling=bool(o['center_sampling']), norm_on_bbox=bool(o['norm_on_bbox']),
                            centerness_on_reg=bool(o['centerness_on_reg']), loss_cls=loss_cls, loss_bbox=loss_bbox,
                            loss_centerness=dict(CTR, loss_weight=wc)).bbox_head
        head.train()
        assert type(head.loss_bbox).__name__ == BOX_TYPES[box] and head.loss_bbox.loss_weight == wb
        assert (head.loss_cls.gamma, head.loss_cls.alpha, head.loss_cls.loss_weight) == (loss_cls['gamma'], loss_cls['alpha'], loss_cls['loss_weight'])
        assert head.loss_centerness.loss_weight == wc and head.cls_convs[0].conv.bias is not None
        seed = sum(map(ord, name))
        rng = np.random.RandomState(seed)
        g = torch.Generator().manual_seed(seed)
        cls, reg, ctr, scales = head_outputs(g, B, not o['norm_on_bbox'], C)
        gtb, gtl, igb = [], [], []
        for i in range(B):
            b, l = gts_for(rng, 128, 192, int(rng.randint(2, 6)), lo=8.0, hi=160.0)
            gtb.append(b)
            gtl.append(l % C)
            igb.append(gts_for(rng, 128, 192, int(rng.randint(0, 4)), lo=8.0, hi=100.0)[0])
        if B == 3:
            gtb[2], gtl[2], igb[2] = gtb[1] / 2, gtl[1], igb[1] / 2
        head.loss_weight, head.soft_weight, head.soft_warm_up, head.cur_iter = lw, sw, 0, 0
        # the reference's own decode line on the raw outputs (fcos_head.py:159-167, training)
        pred = [F.relu(r * scales[i]) if o['norm_on_bbox'] else (r * scales[i]).exp() for i, r in enumerate(reg)]
        losses = head.loss(cls, pred, ctr, gtb, gtl, [dict(img_shape=(128, 192, 3))] * B, gt_bboxes_ignore=igb)
        sum(losses.values()).backward()
        labels, _ = head.get_targets(head.get_points(SIZES, torch.float32, 'cpu'), gtb, gtl)
        num_pos = int((torch.cat(labels) < C).sum())
        assert num_pos >= MIN_POS, (name, num_pos)
        d = dict(sizes=np.array(SIZES), B=B, loss_weight=lw, soft_weight=sw, soft_warm_up=0, with_ig=1, num_pos=num_pos, num_classes=C,
                 scales=scales, gscales=scales.grad, box_loss=np.array(box), box_eps=np.float64(head.loss_bbox.eps),
                 focal_gamma=np.float64(loss_cls['gamma']), focal_alpha=np.float64(loss_cls['alpha']),
                 cls_weight=np.float64(loss_cls['loss_weight']), bbox_weight=np.float64(wb), ctr_weight=np.float64(wc), **o)
        for i in range(B):
            d[f'gt{i}'], d[f'gl{i}'], d[f'ig{i}'] = gtb[i], gtl[i], igb[i]
        for i in range(5):
            d[f'cls{i}'], d[f'reg{i}'], d[f'ctr{i}'] = cls[i], reg[i], ctr[i]
            d[f'gcls{i}'], d[f'greg{i}'], d[f'gctr{i}'] = cls[i].grad, reg[i].grad, ctr[i].grad
        for k, v in losses.items():
            d[k] = np.float64(float(v))
        for k, v in d.items():          # every reference output is finite
            if isinstance(v, torch.Tensor) or k.startswith('loss_'):
                assert bool(torch.isfinite(torch.as_tensor(v)).all()), (name, k)
        print(name, 'num_pos', num_pos, {k: float(v) for k, v in losses.items()})
        save(name + '.npz', **d)


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen()
