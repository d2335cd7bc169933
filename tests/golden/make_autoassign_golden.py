"""Generate the AutoAssign fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_autoassign_golden.py
  autoassign_<case>.npz   the reference's AutoAssignHead (configs/autoassign/autoassign_r50_fpn_8x2_1x_coco.py's bbox_head with GN-32
                          towers) on a 128 x 160 canvas at batch 2: its forward under no_grad on seeded features, its loss with autograd
                          on LEAF COPIES of those outputs (loss.backward() through forward_single fails: `bbox_pred *= stride` modifies
                          a ReLU output in place) and its get_bboxes (with the stand-in NMS of _ref_import.py) - inputs and outputs only.
Cases: a  80 classes, 1-40 random boxes, a trained-looking prior (mean != 0, sigma != 1);  b  the second image without boxes;  c  no
boxes in the batch;  d  a designed first image: two overlapping boxes of one class and one of another class, a box that contains no
point at all ((13, 13, 15, 15): R = 0, the -100 clamp applies) and a box that covers the whole canvas;  e  18 classes, loss weights
0.5 / 1.5 / 0.3, GIoULoss(loss_weight=2).
A case is redrawn (next seed) unless, computed in float64: every box edge is >= 1e-3 from a multiple of 8; every R_g of a box with
inside points lies in (1e-6, 1 - 1e-6); every q <= 1 - 1e-6; and no two kept detections of an image have scores within 1e-5
(relative) of each other, so that their order is not left to the last bits.
Every parameter is seeded (the Conv2d biases are drawn at construction: torch.manual_seed in front of it), then the predictors, the
Scale layers and the prior are redrawn from the case's generator so that ReLU zeros, confident locations and a moved prior occur.
Layout (level-major [level][image][y][x], as the kernels' buffers; per image i the columns are the image's boxes): inside{i} (bool
[P, G_i]), prior{i} (c at the inside pairs, in the mask's row-major order; 0 elsewhere), iou{i} ([P]: the per-point maximum the reference repeats over its boxes, before the inside mask),
negw{i} (the reference's own p_neg_weight [P, C]) - P = 428 points of one image in level order; the head outputs cls{l} / raw{l} (conv_reg's output in
front of Scale; the head's bbox_pred is exactly relu(scale x) s, checked here) / obj{l}, scales, mean, sigma; the three losses and their gradients gcls{l} / gbbox{l} (with respect to bbox_pred) /
gobj{l} / gmean / gsigma; det{i}_boxes (with scores) / det{i}_labels of get_bboxes(rescale=True); head_keys (case a): the reference
head's state_dict keys."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, save  # noqa: E402
import make_paa_golden as MP  # noqa: E402

CFG = '/root/reference/configs/autoassign/autoassign_r50_fpn_8x2_1x_coco.py'
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
STRIDES = (8, 16, 32, 64, 128)
H, W = 128, 160
TEST_CFG = dict(nms_pre=100, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100)
IMG_SHAPES = [(H, W, 3), (100, 130, 3)]
SCALE_FACTORS = [np.ones(4, np.float32), np.full(4, 1.25, np.float32)]


def install():
    MP.install()
    cnn = sys.modules['mmcv.cnn']
    for name in ('normal_init', 'bias_init_with_prob'):      # init_weights is never called here
        if not hasattr(cnn, name):
            setattr(cnn, name, None)
    return importlib.import_module('mmdet.models.dense_heads.autoassign_head')


def build_head(num_classes, seed, **over):
    mod = install()
    hc = dict(R.load_cfg(CFG)['model']['bbox_head'], num_classes=num_classes, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
    hc.pop('type')
    hc.update(over)
    tc = R.AttrDict(TEST_CFG, nms=R.AttrDict(TEST_CFG['nms']))
    torch.manual_seed(seed)
    head = mod.AutoAssignHead(train_cfg=R.AttrDict(), test_cfg=tc, **hc)
    head.train()
    return mod, head


def boxes_for(case, rng, img):
    def rand(n, lo=6.0, hi=110.0):
        w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        x, y = rng.uniform(0, W - 4, n), rng.uniform(0, H - 4, n)
        return np.stack([x, y, np.minimum(x + w, W - 0.5), np.minimum(y + h, H - 0.5)], 1).astype(np.float32)
    if case == 'c' or (case == 'b' and img == 1):
        return np.zeros((0, 4), np.float32)
    if case == 'd' and img == 0:
        j = rng.uniform(-0.2, 0.2, (5, 4))
        b = np.array([[20, 20, 90, 84], [42, 30, 110, 100], [30, 50, 75, 118], [13, 13, 15, 15], [-2, -2, 162, 130]], np.float64) + j
        b[3] = [13, 13, 15, 15]
        return b.astype(np.float32)
    return rand(int(rng.randint(1, 41)) if case == 'a' else int(rng.randint(2, 12)))


def labels_for(case, rng, img, n, C):
    if case == 'd' and img == 0:
        return np.array([3, 3, 7, 3, 5], np.int64)      # boxes 0 and 1 overlap and share class 3: the higher index wins the negative weight
    return rng.randint(0, C, n).astype('int64')


def gen_case(case, seed):
    C = 80 if case == 'a' else 18 if case == 'e' else 20
    over = {}
    if case == 'e':
        over = dict(pos_loss_weight=0.5, neg_loss_weight=1.5, center_loss_weight=0.3, loss_bbox=dict(type='GIoULoss', loss_weight=2.0))
    mod, head = build_head(C, seed, **over)
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        head.conv_cls.weight.normal_(0, 0.04, generator=g); head.conv_cls.bias.normal_(-1.5, 0.3, generator=g)
        head.conv_reg.weight.normal_(0, 0.03, generator=g); head.conv_reg.bias.normal_(0.8, 0.2, generator=g)
        head.conv_centerness.weight.normal_(0, 0.04, generator=g); head.conv_centerness.bias.normal_(0, 0.3, generator=g)
        for s in head.scales:
            s.scale.copy_(1.0 + 0.2 * torch.randn((), generator=g))
        if case != 'c':
            head.center_prior.mean.copy_(0.4 * torch.randn(C, 2, generator=g))
            head.center_prior.sigma.copy_(1.0 + 0.6 * torch.rand(C, 2, generator=g))
    gts = [torch.from_numpy(boxes_for(case, rng, i)) for i in range(2)]
    gls = [torch.from_numpy(labels_for(case, rng, i, len(b), C)) for i, b in enumerate(gts)]
    for b in gts:
        if len(b) and bool(((b.double() / 8 - (b.double() / 8).round()).abs() * 8 < 1e-3).any()):
            return 'a box edge at a multiple of 8'
    feats = [torch.randn(2, 256, h, w, generator=g) for h, w in SIZES]
    raws = []
    hook = head.conv_reg.register_forward_hook(lambda m, i, o: raws.append(o.detach().clone()))
    with torch.no_grad():
        cls, bbox, obj = head(feats)
    hook.remove()
    # (the class logits are rounded to bf16-representable fp32 values before anything reads them: the archive compresses their zero
    # low halves, which keeps case a within the size of the Fovea fixtures)
    cls = [t.detach().bfloat16().float().requires_grad_() for t in cls]
    bbox = [t.detach().clone().requires_grad_() for t in bbox]
    obj = [t.detach().clone().requires_grad_() for t in obj]
    for l in range(5):
        want = torch.relu(raws[l] * head.scales[l].scale.detach()) * STRIDES[l]
        assert torch.equal(want, bbox[l].detach()), 'forward_single: relu(scale x) s'
    metas = [dict(img_shape=s, scale_factor=f) for s, f in zip(IMG_SHAPES, SCALE_FACTORS)]

    # the intermediate quantities, recorded from the reference's own calls
    rec = dict(negw=[], ious=[], inside=[], prior=[])
    o_neg, o_cp = head.get_neg_loss_single, head.center_prior.forward

    class TorchProxy:      # p_neg_weight is the first torch.ones_like of get_neg_loss_single, filled in place (:284,303-304)
        def __getattr__(self, k):
            return getattr(torch, k)

        def ones_like(self, x, **kw):
            t = torch.ones_like(x, **kw)
            ones.append(t)
            return t
    ones = []

    def neg_single(cls_score, objectness, gt_labels, ious, inside):
        rec['ious'].append(ious.detach().clone())
        del ones[:]
        out = o_neg(cls_score, objectness, gt_labels, ious, inside)
        rec['negw'].append(ones[0].detach().clone())
        return out
    mod.torch = TorchProxy()

    def cp_forward(points, gt_bboxes, labels, inside):
        out = o_cp(points, gt_bboxes, labels, inside)
        rec['prior'].append(out[0].detach().clone())
        rec['inside'].append(out[1].detach().clone())
        return out
    head.get_neg_loss_single = neg_single
    head.center_prior.forward = cp_forward
    losses = head.loss(cls, bbox, obj, gts, gls, metas)
    head.get_neg_loss_single = o_neg
    head.center_prior.forward = o_cp
    mod.torch = torch
    sum(losses.values()).backward()

    # float64 restatement of R_g, q and the per-point maximum IoU, for the clean-draw conditions and the stored iou / negw
    pts = torch.cat(head.get_points(SIZES, torch.float32, 'cpu')).double()
    P = len(pts)
    fl = lambda ts, i: torch.cat([t[i].permute(1, 2, 0).reshape(-1, t.shape[1]) for t in ts]).detach()      # noqa: E731
    d = dict(sizes=np.array(SIZES), B=2, num_classes=C, pos_loss_weight=float(head.pos_loss_weight), neg_loss_weight=float(head.neg_loss_weight),
             center_loss_weight=float(head.center_loss_weight), bbox_weight=float(head.loss_bbox.loss_weight),
             scales=np.array([float(s.scale) for s in head.scales], np.float32), mean=head.center_prior.mean.detach(),
             sigma=head.center_prior.sigma.detach(), img_shapes=np.array([s[:2] for s in IMG_SHAPES]), scale_factors=np.stack(SCALE_FACTORS),
             nms_pre=TEST_CFG['nms_pre'], score_thr=TEST_CFG['score_thr'], iou_thr=TEST_CFG['nms']['iou_threshold'],
             max_per_img=TEST_CFG['max_per_img'])
    from mmdet.core.bbox import bbox_overlaps
    for i in range(2):
        G = len(gts[i])
        pc, po, bp = fl(cls, i).double().sigmoid(), fl(obj, i).double().sigmoid(), fl(bbox, i).double()
        dec = torch.stack([pts[:, 0] - bp[:, 0], pts[:, 1] - bp[:, 1], pts[:, 0] + bp[:, 2], pts[:, 1] + bp[:, 3]], 1)
        inside, prior = rec['inside'][i], rec['prior'][i]
        negw = torch.ones(P, C, dtype=torch.float64)
        iou = torch.zeros(P, dtype=torch.float64)
        if G:
            gb = gts[i].double()
            iou = bbox_overlaps(dec, gb).max(1).values
            giou = bbox_overlaps(dec, gb, mode='giou')
            p_pos = pc[:, gls[i]] * po * torch.exp(-float(head.loss_bbox.loss_weight) * (1 - giou))
            wgt = torch.exp(3 * p_pos) * prior.double()
            Rg = (p_pos * wgt).sum(0) / wgt.sum(0).clamp(min=1e-12)
            has = inside.any(0)
            if not bool(((Rg[has] > 1e-6) & (Rg[has] < 1 - 1e-6)).all()):
                return 'an R_g outside (1e-6, 1 - 1e-6)'
            # the reference's fp32 ious (repeated over the boxes, zero outside) must be this maximum at inside pairs
            ref_iou = rec['ious'][i]
            assert bool((ref_iou[inside].double() - iou[:, None].expand(P, G)[inside]).abs().max() < 1e-5) if bool(inside.any()) else True
            for gi in range(G):      # ascending box index: the higher index of a class wins (autoassign_head.py:303-304 on CPU)
                m = inside[:, gi]
                if bool(m.any()):
                    t = 1 / (1 - iou[m]).clamp(min=1e-12)
                    negw[m, int(gls[i][gi])] = 1 - (t - t.min() + 1e-12) / (t.max() - t.min() + 1e-12)
        if not bool(((pc * po * negw) <= 1 - 1e-6).all()):
            return 'a q above 1 - 1e-6'
        d[f'gt{i}'], d[f'gl{i}'] = gts[i], gls[i]
        assert float((rec['negw'][i].double() - negw).abs().max()) < 1e-4, 'p_neg_weight: the float64 restatement and the reference differ'
        assert not bool(prior[~inside].any())
        d[f'inside{i}'], d[f'prior{i}'], d[f'iou{i}'], d[f'negw{i}'] = inside, prior[inside], iou.float(), rec['negw'][i]
    if case == 'd':
        ins = rec['inside'][0]
        assert not bool(ins[:, 3].any()), 'box 3 must contain no point'
        assert bool(ins[:, 4].all()), 'box 4 must contain every point'
        assert bool((ins[:, 0] & ins[:, 1]).any()), 'boxes 0 and 1 must share points'
    with torch.no_grad():
        dets = head.get_bboxes([c.detach() for c in cls], [b.detach() for b in bbox], [o.detach() for o in obj], metas, rescale=True)
    for i in range(2):
        sc = dets[i][0][:, 4].double()
        if len(sc) > 1 and float(((sc[:-1] - sc[1:]) / sc[:-1]).min()) < 1e-5:
            return 'two detections with nearly equal scores'
        d[f'det{i}_boxes'], d[f'det{i}_labels'] = dets[i][0], dets[i][1]
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)      # noqa: E731
    for l in range(5):
        d[f'cls{l}'], d[f'raw{l}'], d[f'obj{l}'] = cls[l].detach(), raws[l], obj[l].detach()
        d[f'gcls{l}'], d[f'gbbox{l}'], d[f'gobj{l}'] = zero(cls[l]), zero(bbox[l]), zero(obj[l])
    d['gmean'], d['gsigma'] = zero(head.center_prior.mean), zero(head.center_prior.sigma)
    for k, v in losses.items():
        d[k] = np.float64(float(v))
        assert np.isfinite(d[k]), k
    if case == 'a':
        d['head_keys'] = np.array(['bbox_head.' + k for k in head.state_dict().keys()])
    print(case, 'seed', seed, 'boxes', [len(b) for b in gts], {k: float(d[k]) for k in losses}, 'dets', [len(x[1]) for x in dets])
    save(f'autoassign_{case}.npz', **d)
    return None


if __name__ == '__main__':
    torch.set_num_threads(8)
    for ci, case in enumerate('abcde'):
        for t in range(50):
            why = gen_case(case, 1000 * (ci + 1) + t)
            if why is None:
                break
            print(case, 'redraw:', why)
        else:
            raise SystemExit(f'case {case}: no clean draw')
