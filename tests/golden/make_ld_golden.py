"""Generate the LD fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_ld_golden.py
  ld_<case>.npz   the reference's LDHead (configs/ld/ld_r18_gflv1_r101_fpn_coco_1x.py's bbox_head / train_cfg) on a 128 x 160 canvas at
                  batch 2: everything make_gfl_golden.py records of GFLHead.loss, through LDHead.loss with autograd, plus the teacher's
                  box logits and Scale values and loss_ld - inputs and outputs only.
Cases: a  80 classes, reg_max 16 (68 logits), T 10, loss_ld.loss_weight 0.25, teacher scales that differ from the student's;  b  an image
with no box (min(npos) == 0);  c  reg_max 15 (64 logits: the one-tile boundary), T 1;  d  reg_max 3, T 2.5, loss_ld.loss_weight 1.0.
b-d have 3 classes.
A case is redrawn (next seed) on make_gfl_golden.py's seven conditions, restated here on the same quantities.  The redraw acts on
inputs alone.
Layout: make_gfl_golden.py's, plus soft{l} (the teacher's box predictor output in front of its Scale, on the same 1 / 8 grid),
soft_scales, T, ld_weight, loss_ld."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, save  # noqa: E402
import make_atss_golden as MA  # noqa: E402
import make_gfl_golden as MG  # noqa: E402

CFG = '/root/reference/configs/ld/ld_r18_gflv1_r101_fpn_coco_1x.py'
SIZES, STRIDES, H, W = MG.SIZES, MG.STRIDES, MG.H, MG.W


def install():
    MG.install()
    imp = importlib.import_module
    imp('mmdet.models.losses.kd_loss')
    return imp('mmdet.models.dense_heads.ld_head')


def build_head(num_classes, reg_max, T=10, ld_weight=0.25):
    mod = install()
    cfg = R.load_cfg(CFG)['model']
    hc = dict(cfg['bbox_head'], num_classes=num_classes, reg_max=reg_max)
    hc.pop('type')
    hc['loss_ld'] = dict(hc['loss_ld'], T=T, loss_weight=ld_weight)
    head = mod.LDHead(train_cfg=R.AttrDict(cfg['train_cfg']), test_cfg=R.AttrDict(cfg['test_cfg']), **hc)
    head.train()
    return head


CASES = dict(a=dict(C=80, reg_max=16), b=dict(C=3, reg_max=16), c=dict(C=3, reg_max=15, T=1), d=dict(C=3, reg_max=3, T=2.5, ld_weight=1.0))


def gen_case(case, seed):
    kw = dict(CASES[case])
    C, reg_max = kw.pop('C'), kw['reg_max']
    head = build_head(C, **kw)
    R_ = reg_max + 1
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    gts = [torch.from_numpy(MG.boxes_for(case, rng, i)) for i in range(2)]
    gls = [torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')) for b in gts]
    pads = [(H, W), (H, W)]
    metas = [dict(img_shape=(p[0], p[1], 3), pad_shape=(p[0], p[1], 3)) for p in pads]
    ref = MA.reference_assignment(head, gts, gls, metas)
    why = MA.check_case(head, gts, ref, 9)
    if why:
        return why
    # head outputs on a grid (class logits in steps of 1 / 256, box logits of 1 / 8): exact fp32 values whose files stay small
    cls = [((torch.randn(2, C, h, w, generator=g) * 1.5 - 2.5) * 256).round().div(256).requires_grad_() for h, w in SIZES]
    reg = [((torch.randn(2, 4 * R_, h, w, generator=g) * 2.0) * 8).round().div(8).requires_grad_() for h, w in SIZES]
    scales = (torch.rand(5, generator=g) * 0.6 + 0.7).requires_grad_()
    soft = [((torch.randn(2, 4 * R_, h, w, generator=g) * 2.0) * 8).round().div(8) for h, w in SIZES]
    soft_scales = torch.rand(5, generator=g) * 0.6 + 0.7
    assert bool((soft_scales != scales.detach()).all())
    pred = [r * scales[i] for i, r in enumerate(reg)]
    soft_pred = [r * soft_scales[i] for i, r in enumerate(soft)]
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
    npos = [int(((img_of == i) & (labels < C)).sum()) for i in range(2)]
    assert num_total == sum(max(n, 1) for n in npos)
    d = dict(sizes=np.array(SIZES), B=2, num_classes=C, reg_max=reg_max, topk=9, anchor_scale=8.0, beta=float(head.loss_cls.beta),
             cls_weight=float(head.loss_cls.loss_weight), bbox_weight=float(head.loss_bbox.loss_weight),
             dfl_weight=float(head.loss_dfl.loss_weight), box_kind=type(head.loss_bbox).__name__, pads=np.array(pads), labels=labels,
             assign_idx=aidx.int(), cls_weight_map=weight, targets=targets, npos=np.array(npos), num_total=int(num_total),
             T=float(head.loss_ld.T), ld_weight=float(head.loss_ld.loss_weight))
    if not len(pos):
        return 'no positive at all'
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
    dist = bbox2distance(ctrs, tgt, reg_max)
    if bool(((dist - dist.round()).abs() < 1e-4).any()):
        return 'a target distance within 1e-4 of an integer'
    if bool((dec == tgt).any()):
        return 'a predicted and a target box share an edge'
    top2 = sig.topk(2, 1)[0]
    if bool((top2[:, 0] == top2[:, 1]).any()):
        return 'two classes tie for the maximum score'
    d.update(pos=pos, decoded=dec, tgt=tgt, score=score, weight=wt, weight_sum=float(wt.sum()), dfl_targets=dist)
    if case == 'b':
        assert min(npos) == 0
    losses = head.loss(cls, pred, gts, gls, soft_pred, metas)
    total = sum(sum(v) for v in losses.values())
    total.backward()
    d.update(scales=scales.detach(), gscales=scales.grad, soft_scales=soft_scales)
    for i in range(2):
        d[f'gt{i}'], d[f'gl{i}'] = gts[i], gls[i]
    for l in range(5):
        d[f'cls{l}'], d[f'reg{l}'], d[f'soft{l}'] = cls[l].detach(), reg[l].detach(), soft[l]
        d[f'gcls{l}'], d[f'greg{l}'] = cls[l].grad, reg[l].grad
    for k, v in losses.items():
        d[k] = np.float64(float(sum(v)))
        assert np.isfinite(d[k]), k
    assert set(losses) == {'loss_cls', 'loss_bbox', 'loss_dfl', 'loss_ld'}
    print(case, 'seed', seed, 'npos', npos, {k: float(d[k]) for k in losses})
    save(f'ld_{case}.npz', **d)
    return None


if __name__ == '__main__':
    torch.set_num_threads(8)
    for ci, case in enumerate('abcd'):
        for t in range(50):
            why = gen_case(case, 3000 * (ci + 1) + t)          # (a redraw reason; the generator's own consistency asserts propagate)
            if why is None:
                break
            print(case, 'redraw:', why)
        else:
            raise SystemExit(f'case {case}: no clean draw')
