"""Torch (CPU) model of the GFL head as include/dsl_hip.h states it (no reference files are read here): the Integral decode, the
quality pass (IoU score, weight, their sum), Quality Focal Loss, the box loss and Distribution Focal Loss in the dtype of their inputs
(float64 with autograd in the tests), and detection by way of tests/aug_ref.py after its own decode.  The assignment is ATSS's
(tests/atss_ref.py).

Everything is level-major [level][image][y][x], as the kernels' buffers are.  test_gfl_cpu.py pins this model to the fixtures
tests/golden/gfl_*.npz, which hold what the reference's own GFLHead.loss computed."""
import numpy as np
import torch

import atss_ref as AR
import aug_ref as A
import loss_family_ref as LF

STRIDES, SIZES = AR.STRIDES, AR.SIZES


def flat_points(sizes, n, strides=STRIDES):
    """[M, 2] anchor centres (x s, y s) and [M] strides, level-major for n images."""
    pts, st = [], []
    for (h, w), s in zip(sizes, strides):
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        p = torch.stack([xs.reshape(-1) * s, ys.reshape(-1) * s], 1).float().repeat(n, 1)
        pts.append(p)
        st.append(torch.full((p.shape[0],), float(s)))
    return torch.cat(pts), torch.cat(st)


def integral(z, reg_max):
    """[K, 4 (reg_max + 1)] scaled logits -> [K, 4] expectations of the per-side softmax over bins 0..reg_max."""
    p = z.reshape(-1, 4, reg_max + 1).softmax(-1)
    return (p * torch.arange(reg_max + 1, dtype=z.dtype)).sum(-1)


def aligned_iou(p, t, eps=1e-6):
    a1, a2 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    wh = (torch.min(p[:, 2:], t[:, 2:]) - torch.max(p[:, :2], t[:, :2])).clamp(min=0)
    ov = wh[:, 0] * wh[:, 1]
    return ov / torch.max(a1 + a2 - ov, ov.new_tensor(eps))


def box_loss(kind, p, t, eps=1e-6):
    return LF.box_loss_elem(kind, p, t, eps)


def decode_pos(raw, scales, asg, sizes, n, reg_max, num_classes, strides=STRIDES):
    """The positives: (pos, decoded prediction, target, point, all in units of the stride, scaled logits z [K, 4 R], level index)."""
    labels = asg['labels']
    lvl = torch.cat([torch.full((n * h * w,), i) for i, (h, w) in enumerate(sizes)])
    pts, st = flat_points(sizes, n, strides)
    pos = (labels < num_classes).nonzero().view(-1)
    z = raw[pos] * scales[lvl[pos]][:, None]
    d = integral(z, reg_max)
    c = (pts[pos] / st[pos][:, None]).to(raw.dtype)
    pred = torch.stack([c[:, 0] - d[:, 0], c[:, 1] - d[:, 1], c[:, 0] + d[:, 2], c[:, 1] + d[:, 3]], 1)
    tgt = asg['targets'].to(raw.dtype)[pos] / st[pos][:, None].to(raw.dtype)
    return pos, pred, tgt, c, z, lvl[pos]


def quality(cls, raw, scales, asg, sizes, n, reg_max, num_classes, strides=STRIDES):
    """score [M], weight [M] (0 off the positives) and the sum of the weights, in the dtype of the inputs."""
    M = cls.shape[0]
    score, weight = torch.zeros(M, dtype=cls.dtype), torch.zeros(M, dtype=cls.dtype)
    pos, pred, tgt, *_ = decode_pos(raw.detach(), scales.detach(), asg, sizes, n, reg_max, num_classes, strides)
    if len(pos):
        score[pos] = aligned_iou(pred, tgt)
        weight[pos] = cls.detach()[pos].sigmoid().max(1)[0]
    return score, weight, weight.sum()


def dfl_targets(c, tgt, reg_max):
    """bbox2distance (transforms.py:165-186): [K, 4] side distances clamped to [0, reg_max - 0.1]."""
    t = torch.stack([c[:, 0] - tgt[:, 0], c[:, 1] - tgt[:, 1], tgt[:, 2] - c[:, 0], tgt[:, 3] - c[:, 1]], 1)
    return t.clamp(min=0, max=reg_max - 0.1)


def loss(cls, raw, scales, asg, sizes, n, num_classes=80, reg_max=16, beta=2.0, cls_weight=1.0, bbox_weight=2.0, dfl_weight=0.25,
         box_kind='giou', box_eps=1e-6, world=1.0, norm=None, strides=STRIDES):
    """Losses of flat level-major head outputs: cls [M, C], raw [M, 4 (reg_max + 1)] (the box predictor's output, in front of Scale),
    scales [5]; `asg` from atss_ref.assign().  norm = (sum of num_total over ranks, sum of the weight sums over ranks), default this
    rank's.  Returns (loss_cls, loss_bbox, loss_dfl) graph-connected, and (score, weight, weight sum)."""
    labels, lw = asg['labels'], asg['cls_weight'].to(cls.dtype)
    score, weight, wsum = quality(cls, raw, scales, asg, sizes, n, reg_max, num_classes, strides)
    tot, ws = (float(asg['num_total']), float(wsum)) if norm is None else norm
    num, avg = max(tot / world, 1.0), max(ws / world, 1.0)
    p = cls.sigmoid()
    zero = torch.zeros_like(cls)
    l = torch.nn.functional.binary_cross_entropy_with_logits(cls, zero, reduction='none') * p.pow(beta)
    pos, pred, tgt, c, z, _ = decode_pos(raw, scales, asg, sizes, n, reg_max, num_classes, strides)
    if len(pos):
        xl = cls[pos, labels[pos]]
        lp = torch.nn.functional.binary_cross_entropy_with_logits(xl, score[pos], reduction='none') * (score[pos] - xl.sigmoid()).abs().pow(beta)
        keep = torch.ones_like(cls)
        keep[pos, labels[pos]] = 0.0
        l_cls = ((l * keep).sum(1) * lw).sum() + (lp * lw[pos]).sum()
    else:
        l_cls = (l.sum(1) * lw).sum()
    l_cls = l_cls / num * cls_weight
    if len(pos) == 0:
        return l_cls, raw.sum() * 0, raw.sum() * 0, (score, weight, wsum)
    wp = weight[pos]
    l_box = (box_loss(box_kind, pred, tgt, box_eps) * wp).sum() / avg * bbox_weight
    t = dfl_targets(c, tgt, reg_max).reshape(-1)
    left = t.long()
    zz = z.reshape(-1, reg_max + 1)
    ce = torch.nn.functional.cross_entropy
    dfl = ce(zz, left, reduction='none') * (left + 1 - t) + ce(zz, left + 1, reduction='none') * (t - left)
    l_dfl = (dfl.reshape(-1, 4).sum(1) * wp).sum() / (4.0 * avg) * dfl_weight
    return l_cls, l_box, l_dfl, (score, weight, wsum)


def collect(cls, raw, scales, img_shape, scale_factor, flip_direction, nms_pre, reg_max, strides=STRIDES):
    """aug_ref.collect with the GFL decode: one view ([1, ., h, w] per level) -> mapped-back boxes [R, 4], scores [R, C] and a unit
    centerness [R] (the candidate score is the class sigmoid alone)."""
    boxes, scores = [], []
    H, W = float(img_shape[0]), float(img_shape[1])
    for l, (c, r, s) in enumerate(zip(cls, raw, strides)):
        h, w = c.shape[2:]
        P = h * w
        sc = c[0].permute(1, 2, 0).reshape(P, -1).sigmoid()
        z = r[0].permute(1, 2, 0).reshape(P, -1) * scales[l]
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        pt = torch.stack([xs.reshape(-1) * s, ys.reshape(-1) * s], 1).float()
        if 0 < nms_pre < P:
            idx = sc.max(1)[0].sort(descending=True, stable=True)[1][:nms_pre].sort()[0]
            sc, z, pt = sc[idx], z[idx], pt[idx]
        d = integral(z, reg_max) * s
        b = torch.stack([(pt[:, 0] - d[:, 0]).clamp(0, W), (pt[:, 1] - d[:, 1]).clamp(0, H), (pt[:, 0] + d[:, 2]).clamp(0, W),
                         (pt[:, 1] + d[:, 3]).clamp(0, H)], 1)
        boxes.append(b)
        scores.append(sc)
    b = torch.cat(boxes)
    if flip_direction in ('horizontal', 'diagonal'):
        b = torch.stack([W - b[:, 2], b[:, 1], W - b[:, 0], b[:, 3]], 1)
    if flip_direction in ('vertical', 'diagonal'):
        b = torch.stack([b[:, 0], H - b[:, 3], b[:, 2], H - b[:, 1]], 1)
    s = torch.cat(scores)
    return b / torch.tensor(np.asarray(scale_factor, np.float32)), s, torch.ones(s.shape[0])


def detect(cls, raw, scales, img_shapes, reg_max, nms_pre=1000, score_thr=0.05, iou_thr=0.6, max_per_img=100):
    """Per image (dets [k, 5], labels [k]) through aug_ref.finish (detect_ref's rules), no rescale."""
    out = []
    for i in range(cls[0].shape[0]):
        view = [[x[i:i + 1] for x in t] for t in (cls, raw)]
        b, s, c = collect(*view, scales, img_shapes[i], np.ones(4, np.float32), None, nms_pre, reg_max)
        out.append(A.finish(b, s, c, score_thr=score_thr, iou_thr=iou_thr, max_per_img=max_per_img, cap=16384)[:2])
    return out
