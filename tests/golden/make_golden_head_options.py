"""Generate the head-option fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_golden_head_options.py
  assign_plain_{small,full}.npz   FCOSHead.get_targets with center_sampling=False on the crafted boxes / canvases of make_golden.gen_assign
                                  (tie, point on a box edge, degenerate box): labels, the un-normalised targets (norm_on_bbox=False) and
                                  the normalised ones (norm_on_bbox=True)
  loss_plain_{sup,sup_ig,dsl,nopos}.npz   FCOSHead.loss of the plain head (configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_coco.py) on the
                                  128 x 192 canvas of make_golden.gen_loss
  loss_opt_<option>.npz           the tricks head with ONE option flipped; loss_opt_centerness_on_reg_c18: that flip on an 18-class
                                  head, DSL batch of three (C % 4 != 0 next to the centerness column)
  net_tiny_plain.npz              the whole plain model at 2 x 64 x 96: losses, head outputs, gradient norms and keys as net_tiny
  sweep_tiny_plain.npz            simple_test of the plain model (exp decode, centerness on the classification tower)
The loss fixtures hold the RAW regression outputs `reg` and the Scale parameters `scales`: bbox_pred = relu(scale * reg) or exp(scale *
reg) is formed here with the reference's own line (fcos_head.py:159-167), so `greg` / `gscales` are gradients through it.  Size rule (no fixture larger than the largest existing file of its kind), as read here: kinds are assign_* (largest assign_full.npz),
loss_* (loss_dsl.npz), net_* (net_small_dsl.npz) and the detection fixtures sweep_tiny / bboxes_synth / detect_many (largest
bboxes_synth.npz).  Every loss
fixture except the no-positives one holds at least MIN_POS positive locations (asserted here, stored as `num_pos`).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, O, SUP_CFG, gts_for, save  # noqa: E402

PLAIN_CFG = '/root/reference/configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_coco.py'
MIN_POS = 20
IOU = dict(type='IoULoss', loss_weight=1.0)
# name -> (reference config, head overrides, the options the fixture records)
PLAIN = dict(center_sampling=0, norm_on_bbox=0, centerness_on_reg=0, iou_loss=1, conv_bias=0)
TRICKS = dict(center_sampling=1, norm_on_bbox=1, centerness_on_reg=1, iou_loss=0, conv_bias=1)
FLIPS = dict(center_sampling=dict(center_sampling=False), norm_on_bbox=dict(norm_on_bbox=False),
             centerness_on_reg=dict(centerness_on_reg=False), iou_loss=dict(loss_bbox=IOU), conv_bias=dict(conv_bias='auto'))
SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]       # 128 x 192 canvas


def opts_of(flip=None):
    if flip is None:
        return dict(PLAIN)
    o = dict(TRICKS)
    o[flip] = 1 - o[flip]
    return o


def gen_assign():
    cs_off_raw = R.build_fcos(PLAIN_CFG).bbox_head
    cs_off_norm = R.build_fcos(PLAIN_CFG, norm_on_bbox=True).bbox_head
    assert not cs_off_raw.center_sampling and not cs_off_raw.norm_on_bbox and cs_off_norm.norm_on_bbox
    sizes = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
    gtb = [torch.tensor([[0., 0., 64., 64.], [32., 32., 96., 96.], [0., 0., 64., 64.],   # tie 0/2
                         [4., 4., 20., 20.], [4., 4., 36., 36.], [60., 20., 60., 90.],    # (point 4, 4 / 20, 20 on an edge; degenerate box)
                         [10., 12., 150., 120.], [100., 4., 108., 12.]]),
           torch.zeros(0, 4),
           torch.tensor([[12., 12., 28., 28.], [12., 12., 28., 28.]])]
    gtl = [torch.tensor([1, 2, 3, 4, 5, 6, 7, 8]), torch.zeros(0, dtype=torch.long), torch.tensor([9, 10])]
    rng = np.random.RandomState(2024)
    fb, fl = [], []
    for n in (7, 40):
        b, l = gts_for(rng, 800, 1333, n, lo=16.0, hi=600.0)
        fb.append(b)
        fl.append(l)
    for name, sz, boxes, labs in (('assign_plain_small.npz', sizes, gtb, gtl),
                                  ('assign_plain_full.npz', [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)], fb, fl)):
        pts = cs_off_raw.get_points(sz, torch.float32, 'cpu')
        labels, tg = cs_off_raw.get_targets(pts, boxes, labs)
        labels_n, tg_n = cs_off_norm.get_targets(pts, boxes, labs)
        assert all(torch.equal(a, b) for a, b in zip(labels, labels_n))
        # (targets stored transposed, [4][M]: each of l, t, r, b varies smoothly along a row, which is what keeps the file small)
        d = dict(sizes=np.array(sz), n_img=len(boxes), labels=torch.cat(labels).to(torch.int16),
                 bbox_targets_t=torch.cat(tg).t().contiguous(), bbox_targets_norm_t=torch.cat(tg_n).t().contiguous())
        for i, (b, l) in enumerate(zip(boxes, labs)):
            d[f'gt{i}'], d[f'gl{i}'] = b, l
        save(name, **d)


def head_outputs(g, B, exp_decode, C=80):
    cls = [(torch.randn(B, C, h, w, generator=g) * 1.5 - 2.0).requires_grad_() for h, w in SIZES]
    if exp_decode:      # exp(scale * reg) in pixels: e^0 .. e^5
        reg = [(torch.rand(B, 4, h, w, generator=g) * 5.0).requires_grad_() for h, w in SIZES]
    else:               # relu(scale * reg) in strides; a tenth of the entries negative or zero
        reg = [((torch.rand(B, 4, h, w, generator=g) * 6.0 - 0.3) * (torch.rand(B, 4, h, w, generator=g) > 0.1)).requires_grad_()
               for h, w in SIZES]
    ctr = [torch.randn(B, 1, h, w, generator=g).requires_grad_() for h, w in SIZES]
    scales = (torch.rand(5, generator=g) * 0.5 + 0.75).requires_grad_()
    return cls, reg, ctr, scales


def gen_loss():
    legs = [('loss_plain_sup', None, 2, 1.0, 0.0, False, False), ('loss_plain_sup_ig', None, 2, 1.0, 0.0, True, False),
            ('loss_plain_dsl', None, 3, 3.0, 1.0, True, False), ('loss_plain_nopos', None, 2, 1.0, 0.0, False, True)]
    legs += [(f'loss_opt_{k}', k, 2, 1.0, 0.0, True, False) for k in FLIPS]
    # 18 classes (C % 4 != 0: the last group of four is partial) with the centerness logit on the classification tower
    legs += [('loss_opt_centerness_on_reg_c18', 'centerness_on_reg', 3, 3.0, 1.0, True, False)]
    for name, flip, B, lw, sw, with_ig, nopos in legs:
        C = 18 if name.endswith('_c18') else 80
        kw = dict(num_classes=C) if C != 80 else {}
        head = (R.build_fcos(PLAIN_CFG) if flip is None else R.build_fcos(SUP_CFG, **FLIPS[flip], **kw)).bbox_head
        head.train()
        o = opts_of(flip)
        assert (int(head.center_sampling), int(head.norm_on_bbox), int(head.centerness_on_reg), int(type(head.loss_bbox).__name__ == 'IoULoss'),
                int(head.cls_convs[0].conv.bias is not None)) == tuple(o[k] for k in ('center_sampling', 'norm_on_bbox', 'centerness_on_reg',
                                                                                        'iou_loss', 'conv_bias')), name
        seed = sum(map(ord, name))
        rng = np.random.RandomState(seed)
        g = torch.Generator().manual_seed(seed)
        cls, reg, ctr, scales = head_outputs(g, B, not o['norm_on_bbox'], C)
        gtb, gtl, igb = [], [], []
        for i in range(B):
            b, l = gts_for(rng, 128, 192, 0 if nopos else int(rng.randint(2, 6)), lo=8.0, hi=160.0)
            gtb.append(b)
            gtl.append(l % C)
            igb.append(gts_for(rng, 128, 192, int(rng.randint(0, 4)), lo=8.0, hi=100.0)[0])
        if B == 3:
            gtb[2], gtl[2], igb[2] = gtb[1] / 2, gtl[1], igb[1] / 2
        head.loss_weight, head.soft_weight, head.soft_warm_up, head.cur_iter = lw, sw, 0, 0
        # the reference's own decode line on the raw outputs (fcos_head.py:159-167, training)
        pred = [F.relu(r * scales[i]) if o['norm_on_bbox'] else (r * scales[i]).exp() for i, r in enumerate(reg)]
        losses = head.loss(cls, pred, ctr, gtb, gtl, [dict(img_shape=(128, 192, 3))] * B, gt_bboxes_ignore=igb if with_ig else None)
        sum(losses.values()).backward()
        labels, _ = head.get_targets(head.get_points(SIZES, torch.float32, 'cpu'), gtb, gtl)
        num_pos = int((torch.cat(labels) < C).sum())
        assert (num_pos == 0) if nopos else (num_pos >= MIN_POS), (name, num_pos)
        d = dict(sizes=np.array(SIZES), B=B, loss_weight=lw, soft_weight=sw, soft_warm_up=0, with_ig=int(with_ig), num_pos=num_pos, num_classes=C,
                 scales=scales, gscales=scales.grad, **o)
        for i in range(B):
            d[f'gt{i}'], d[f'gl{i}'], d[f'ig{i}'] = gtb[i], gtl[i], igb[i]
        for i in range(5):
            d[f'cls{i}'], d[f'reg{i}'], d[f'ctr{i}'] = cls[i], reg[i], ctr[i]
            d[f'gcls{i}'], d[f'greg{i}'], d[f'gctr{i}'] = cls[i].grad, reg[i].grad, ctr[i].grad
        for k, v in losses.items():
            d[k] = np.float64(float(v))
        print(name, 'num_pos', num_pos, {k: float(v) for k, v in losses.items()})
        save(name + '.npz', **d)


def plain_sd():
    return {k: v for k, v in O.synth_state_dict(0).items()
            if not (k.startswith(('bbox_head.cls_convs.', 'bbox_head.reg_convs.')) and k.endswith('.conv.bias'))}


def gen_net():
    model = R.build_fcos(PLAIN_CFG)
    sd = plain_sd()
    print('load_state_dict', model.load_state_dict(sd, strict=True))
    model.train()
    tk = O.trainable_keys(sd)
    assert sorted(tk) == sorted(k for k, p in model.named_parameters() if p.requires_grad)
    rng = np.random.RandomState(11)
    B, H, W = 2, 64, 96
    g = torch.Generator().manual_seed(5 + B + H)
    img = torch.randn(B, 3, H, W, generator=g) * 40.0
    gtb, gtl = [], []
    for i in range(B):
        b, l = gts_for(rng, H, W, int(rng.randint(2, 4)), lo=8.0, hi=80.0)
        gtb.append(b)
        gtl.append(l)
    model.zero_grad()
    metas = [dict(img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0)] * B
    outs = model.bbox_head(model.extract_feat(img))
    losses = model.bbox_head.loss(*outs, gtb, gtl, metas, gt_bboxes_ignore=None)
    sum(losses.values()).backward()
    d = dict(img=img, B=B, **PLAIN)
    for i in range(B):
        d[f'gt{i}'], d[f'gl{i}'] = gtb[i], gtl[i]
    for i in range(5):
        d[f'cls{i}'], d[f'reg{i}'], d[f'ctr{i}'] = outs[0][i], outs[1][i], outs[2][i]
    for k, v in losses.items():
        d[k] = np.float64(float(v))
    named = dict(model.named_parameters())
    d['state_keys'] = np.array(sorted(model.state_dict()))
    d['grad_keys'] = np.array(tk)
    d['grad_norms'] = np.array([float(named[k].grad.norm()) for k in tk], dtype=np.float64)
    for k in ('bbox_head.conv_reg.weight', 'bbox_head.conv_centerness.weight', 'bbox_head.conv_cls.bias', 'bbox_head.scales.0.scale',
              'bbox_head.scales.3.scale', 'bbox_head.cls_convs.3.gn.weight', 'neck.lateral_convs.2.conv.bias'):
        d['grad/' + k] = named[k].grad
    print({k: float(v) for k, v in losses.items()})
    save('net_tiny_plain.npz', **d)
    # test time: exp decode, centerness from the classification tower; the focal prior raised so that scores pass score_thr
    sd2 = dict(sd)
    sd2['bbox_head.conv_cls.bias'] = torch.full((80,), -1.5)
    sd2['bbox_head.conv_reg.bias'] = sd['bbox_head.conv_reg.bias'] + 2.0        # exp(scale * x): boxes of e^3 = 20 pixels
    model.load_state_dict(sd2, strict=True)
    model.eval()
    g = torch.Generator().manual_seed(99)
    img = torch.randn(2, 3, 96, 128, generator=g) * 40.0
    sf = np.array([1.25, 1.25, 1.25, 1.25], dtype=np.float32)
    metas = [dict(img_shape=(90, 120, 3), pad_shape=(96, 128, 3), scale_factor=sf)] * 2
    with torch.no_grad():
        outs = model.bbox_head(model.extract_feat(img))
        dets = model.bbox_head.get_bboxes(*outs, metas, rescale=True)
    d = dict(img=img, scale_factor=sf, img_shape=np.array([90, 120, 3]), cls_bias=-1.5, reg_bias_add=2.0, **PLAIN)
    for i in range(5):
        d[f'cls{i}'], d[f'reg{i}'], d[f'ctr{i}'] = outs[0][i], outs[1][i], outs[2][i]
    for i, (b, l) in enumerate(dets):
        d[f'det{i}'], d[f'lab{i}'] = b, l
        print('dets', i, b.shape)
    save('sweep_tiny_plain.npz', **d)


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_assign()
    gen_loss()
    gen_net()
