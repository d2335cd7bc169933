"""Generate the GFL fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_gfl_golden.py
  gfl_<case>.npz   the reference's GFLHead (configs/gfl/gfl_r50_fpn_1x_coco.py's bbox_head / train_cfg) on a 128 x 160 canvas at batch 2:
                   its anchors, ATSSAssigner targets, Integral, bbox_overlaps, QualityFocalLoss, the box loss and DistributionFocalLoss
                   through GFLHead.loss with autograd - inputs and outputs only.
Cases: a  1-40 random boxes, reg_max 16, 80 classes (68 box logits: the two-tile predictor);  b  an image with no box;  c  reg_max 15 (64
logits: the one-tile boundary);  d  reg_max 3 with a 60-100 px box: some target distances are clamped at reg_max - 0.1, some are not
(asserted);  e  the second image with pad_shape (96, 128);  f  beta 1.5, loss_dfl.loss_weight 0.5, DIoULoss.  b-f have 3 classes (the
partial class group).
A case is redrawn (next seed) on the four conditions of make_atss_golden.py and when (5) a positive's target distance lies within
1e-4 of an integer (the kink of floor), (6) a predicted and a target box have an equal edge (the kink of min / max in IoU / GIoU) or
(7) two classes tie for a positive's maximum score.  The redraw acts on inputs alone.
Layout (level-major [level][image][y][x]): labels, assign_idx, cls_weight, targets (the assigned box), npos, num_total; the head outputs
cls{l} / reg{l} (the box predictor's output in front of Scale), scales; the three losses, their gradients, and of the positives the
decoded prediction / target in stride units, the IoU score, the weight, the clamped DFL targets; the weight sum."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, save  # noqa: E402
import make_atss_golden as MA  # noqa: E402

CFG = '/root/reference/configs/gfl/gfl_r50_fpn_1x_coco.py'
SIZES, STRIDES, H, W = MA.SIZES, MA.STRIDES, MA.H, MA.W


def install():
    MA.install()
    imp = importlib.import_module
    core = sys.modules['mmdet.core']
    tr = imp('mmdet.core.bbox.transforms')
    for n in ('bbox2distance', 'distance2bbox'):
        if not hasattr(core, n):
            setattr(core, n, getattr(tr, n))
    if not hasattr(core, 'bbox_overlaps'):
        core.bbox_overlaps = imp('mmdet.core.bbox.iou_calculators.iou2d_calculator').bbox_overlaps
    imp('mmdet.models.losses.gfocal_loss')
    for n in ('iou_loss',):
        imp('mmdet.models.losses.' + n)
    return imp('mmdet.models.dense_heads.gfl_head')


def build_head(num_classes, reg_max, beta=2.0, dfl_weight=0.25, loss_bbox=None):
    mod = install()
    cfg = R.load_cfg(CFG)['model']
    hc = dict(cfg['bbox_head'], num_classes=num_classes, reg_max=reg_max)
    hc.pop('type')
    hc['loss_cls'] = dict(hc['loss_cls'], beta=beta)
    hc['loss_dfl'] = dict(hc['loss_dfl'], loss_weight=dfl_weight)
    if loss_bbox is not None:
        hc['loss_bbox'] = loss_bbox
    head = mod.GFLHead(train_cfg=R.AttrDict(cfg['train_cfg']), test_cfg=R.AttrDict(cfg['test_cfg']), **hc)
    head.train()
    return head


def boxes_for(case, rng, img):
    if case == 'd':          # reg_max 3: a 60-100 px box reaches past 2.9 strides on the fine levels
        b = MA.boxes_for('x', rng, img)
        w, h = rng.uniform(60, 100), rng.uniform(60, 100)
        x, y = rng.uniform(0, W - w - 1), rng.uniform(0, H - h - 1)
        b[0] = (x, y, x + w, y + h)
        return b
    return MA.boxes_for(case if case in 'ab' else 'x', rng, img)


CASES = dict(a=dict(C=80, reg_max=16), b=dict(C=3, reg_max=16), c=dict(C=3, reg_max=15), d=dict(C=3, reg_max=3), e=dict(C=3, reg_max=16),
             f=dict(C=3, reg_max=16, beta=1.5, dfl_weight=0.5, loss_bbox=dict(type='DIoULoss', loss_weight=2.0)))


def gen_case(case, seed):
    kw = dict(CASES[case])
    C, reg_max = kw.pop('C'), kw['reg_max']
    head = build_head(C, **kw)
    R_ = reg_max + 1
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    gts = [torch.from_numpy(boxes_for(case, rng, i)) for i in range(2)]
    gls = [torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')) for b in gts]
    pads = [(H, W), (96, 128) if case == 'e' else (H, W)]
    metas = [dict(img_shape=(p[0], p[1], 3), pad_shape=(p[0], p[1], 3)) for p in pads]
    ref = MA.reference_assignment(head, gts, gls, metas)
    why = MA.check_case(head, gts, ref, 9)
    if why:
        return why
    # head outputs on a grid (class logits in steps of 1 / 256, box logits of 1 / 8): exact fp32 values whose files stay small
    cls = [((torch.randn(2, C, h, w, generator=g) * 1.5 - 2.5) * 256).round().div(256).requires_grad_() for h, w in SIZES]
    reg = [((torch.randn(2, 4 * R_, h, w, generator=g) * 2.0) * 8).round().div(8).requires_grad_() for h, w in SIZES]
    scales = (torch.rand(5, generator=g) * 0.6 + 0.7).requires_grad_()
    pred = [r * scales[i] for i, r in enumerate(reg)]
    # targets in the kernels' layout
    anchor_list, valid_list = head.get_anchors(SIZES, metas, device='cpu')
    tg = head.get_targets(anchor_list, valid_list, gts, metas, gt_labels_list=gls, label_channels=C)
    _, labels_l, lw_l, bt_l, _, num_total, _ = tg
    labels = torch.cat([x.reshape(-1) for x in labels_l])
    weight = torch.cat([x.reshape(-1) for x in lw_l])
    targets = torch.cat([x.reshape(-1, 4) for x in bt_l])
    split = [h * w for h, w in SIZES]
    per = [r[3].split(split) for r in ref]
    aidx = torch.cat([per[i][l] for l in range(5) for i in range(2)])
    img_of = torch.cat([torch.cat([torch.full((split[l],), i) for i in range(2)]) for l in range(5)])
    st = torch.cat([torch.full((2 * split[l],), float(STRIDES[l])) for l in range(5)])
    pos = (labels < C).nonzero().view(-1)
    assert torch.equal(pos, (aidx >= 0).nonzero().view(-1))
    for m in pos.tolist():
        i = int(img_of[m])
        assert torch.equal(targets[m], gts[i][aidx[m]]) and int(labels[m]) == int(gls[i][aidx[m]])
    npos = [int(((img_of == i) & (labels < C)).sum()) for i in range(2)]
    assert num_total == sum(max(n, 1) for n in npos)
    d = dict(sizes=np.array(SIZES), B=2, num_classes=C, reg_max=reg_max, topk=9, anchor_scale=8.0, beta=float(head.loss_cls.beta),
             cls_weight=float(head.loss_cls.loss_weight), bbox_weight=float(head.loss_bbox.loss_weight),
             dfl_weight=float(head.loss_dfl.loss_weight), box_kind=type(head.loss_bbox).__name__, pads=np.array(pads), labels=labels,
             assign_idx=aidx.int(), cls_weight_map=weight, targets=targets, npos=np.array(npos), num_total=int(num_total))
    if len(pos):
        from mmdet.core import bbox2distance, bbox_overlaps, distance2bbox
        fresh = head.get_anchors(SIZES, metas, device='cpu')[0]
        anchors_lm = torch.cat([torch.cat([fresh[i][l] for i in range(2)]) for l in range(5)])
        flat_pred = torch.cat([p.permute(0, 2, 3, 1).reshape(-1, 4 * R_) for p in pred]).detach()
        flat_cls = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, C) for c in cls]).detach()
        ctrs = head.anchor_center(anchors_lm[pos]) / st[pos][:, None]
        dec = distance2bbox(ctrs, head.integral(flat_pred[pos]))
        tgt = targets[pos] / st[pos][:, None]
        score = bbox_overlaps(dec, tgt, is_aligned=True)
        sig = flat_cls[pos].sigmoid()
        wt = sig.max(1)[0]
        raw_t = torch.stack([ctrs[:, 0] - tgt[:, 0], ctrs[:, 1] - tgt[:, 1], tgt[:, 2] - ctrs[:, 0], tgt[:, 3] - ctrs[:, 1]], 1)
        dist = bbox2distance(ctrs, tgt, reg_max)
        if bool(((dist - dist.round()).abs() < 1e-4).any()):
            return 'a target distance within 1e-4 of an integer'
        if bool((dec == tgt).any()):
            return 'a predicted and a target box share an edge'
        top2 = sig.topk(2, 1)[0]
        if bool((top2[:, 0] == top2[:, 1]).any()):
            return 'two classes tie for the maximum score'
        if case == 'd':
            clamped = raw_t > reg_max - 0.1
            if not (bool(clamped.any()) and bool((~clamped).any())):
                return 'reg_max 3: both clamped and unclamped target distances are needed'
        d.update(pos=pos, decoded=dec, tgt=tgt, score=score, weight=wt, weight_sum=float(wt.sum()), dfl_targets=dist)
    else:
        d.update(pos=np.zeros(0, np.int64), weight_sum=0.0)
    if case == 'b':
        assert min(npos) == 0
    losses = head.loss(cls, pred, gts, gls, metas)
    total = sum(sum(v) for v in losses.values())
    total.backward()
    d.update(scales=scales.detach(), gscales=scales.grad)
    for i in range(2):
        d[f'gt{i}'], d[f'gl{i}'] = gts[i], gls[i]
    for l in range(5):
        d[f'cls{l}'], d[f'reg{l}'] = cls[l].detach(), reg[l].detach()
        d[f'gcls{l}'], d[f'greg{l}'] = cls[l].grad, reg[l].grad
    for k, v in losses.items():
        d[k] = np.float64(float(sum(v)))
        assert np.isfinite(d[k]), k
    print(case, 'seed', seed, 'npos', npos, {k: float(d[k]) for k in losses})
    save(f'gfl_{case}.npz', **d)
    return None


if __name__ == '__main__':
    torch.set_num_threads(8)
    for ci, case in enumerate('abcdef'):
        for t in range(50):
            why = gen_case(case, 2000 * (ci + 1) + t)          # (a redraw reason; the generator's own consistency asserts propagate)
            if why is None:
                break
            print(case, 'redraw:', why)
        else:
            raise SystemExit(f'case {case}: no clean draw')
