"""Torch (CPU) model of the ATSS head as include/dsl_hip.h states it (no reference files are read here): the assignment in fp32 with
the kernel's documented tie rules, the anchor-delta decode, the three losses in float64 with autograd, and detection by way of
tests/aug_ref.py / tests/detect_ref.py after its own decode.

Everything is level-major [level][image][y][x], as the kernels' buffers are.  test_atss_cpu.py pins this model to the fixtures
tests/golden/atss_*.npz, which hold what the reference's own ATSSAssigner / DeltaXYWHBBoxCoder / ATSSHead.loss computed."""
import math

import numpy as np
import torch

import aug_ref as A

STRIDES = (8, 16, 32, 64, 128)
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]          # the 128 x 160 canvas: two levels have fewer than 9 anchors
MAX_RATIO = abs(math.log(16 / 1000))                         # wh_ratio_clip of delta2bbox
STDS = (0.1, 0.1, 0.2, 0.2)


def level_anchors(sizes, anchor_scale=8.0, strides=STRIDES):
    """Per level [h * w, 4] fp32: location (x, y) -> [x s - a/2, y s - a/2, x s + a/2, y s + a/2], a = anchor_scale * s."""
    out = []
    for (h, w), s in zip(sizes, strides):
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        sx, sy = (xs.reshape(-1) * s).float(), (ys.reshape(-1) * s).float()
        hw = torch.tensor(0.5 * (s * float(anchor_scale)), dtype=torch.float32)
        out.append(torch.stack([sx - hw, sy - hw, sx + hw, sy + hw], 1))
    return out


def valid_masks(sizes, pad_shape, strides=STRIDES):
    """Per level [h * w] bool: x < min(ceil(pad_w / s), w) and y < min(ceil(pad_h / s), h)."""
    out = []
    for (h, w), s in zip(sizes, strides):
        vh, vw = min(-(-int(pad_shape[0]) // s), h), min(-(-int(pad_shape[1]) // s), w)
        m = torch.zeros(h, w, dtype=torch.bool)
        m[:vh, :vw] = True
        out.append(m.reshape(-1))
    return out


def iou_matrix(a, b):
    """BboxOverlaps2D, mode 'iou': [len(a), len(b)], union clamped at 1e-6 (dtype of the inputs)."""
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[None, :, 2:]) - torch.max(a[:, None, :2], b[None, :, :2])).clamp(min=0)
    ov = wh[..., 0] * wh[..., 1]
    return ov / torch.max(a1[:, None] + a2[None, :] - ov, ov.new_tensor(1e-6))


def assign_image(sizes, gt, gl, pad_shape, topk=9, anchor_scale=8.0, num_classes=80, strides=STRIDES):
    """One image.  Returns per-location tensors over the image's locations in level order: labels, assign_idx (-1 = none),
    cls_weight, targets (the assigned box, zeros elsewhere), and `cands` = [(level, location index, IoU, threshold)] per box."""
    anchors, valid = level_anchors(sizes, anchor_scale, strides), valid_masks(sizes, pad_shape, strides)
    P = sum(h * w for h, w in sizes)
    labels = torch.full((P,), num_classes, dtype=torch.long)
    aidx = torch.full((P,), -1, dtype=torch.int32)
    weight = torch.cat(valid).float()
    targets = torch.zeros(P, 4)
    gt = gt.reshape(-1, 4).float()
    best_iou = torch.full((P,), -1.0)
    cands = []
    start = np.cumsum([0] + [h * w for h, w in sizes])
    for g in range(gt.shape[0]):
        gcx, gcy = (gt[g, 0] + gt[g, 2]) / 2.0, (gt[g, 1] + gt[g, 3]) / 2.0
        sel = []
        for l, (a, v) in enumerate(zip(anchors, valid)):
            idx = v.nonzero().view(-1)
            if len(idx) == 0:
                continue
            cx, cy = (a[idx, 0] + a[idx, 2]) / 2.0, (a[idx, 1] + a[idx, 3]) / 2.0
            d = ((cx - gcx).pow(2) + (cy - gcy).pow(2)).sqrt()
            k = min(topk, len(idx))
            order = d.sort(stable=True)[1][:k]           # ties: the lower anchor index
            sel += [(l, int(i)) for i in idx[order]]
        box = torch.stack([anchors[l][i] for l, i in sel])
        iou = iou_matrix(box, gt[g:g + 1])[:, 0]
        s = torch.zeros((), dtype=torch.float32)
        for v in iou:                                    # ascending (level, rank) order, fp32
            s = s + v
        mean = s / len(iou)
        ss = torch.zeros((), dtype=torch.float32)
        for v in iou:
            ss = ss + (v - mean) * (v - mean)
        thr = mean + (ss / torch.tensor(float(len(iou) - 1))).sqrt() if len(iou) > 1 else torch.tensor(float('nan'))
        cands.append([(l, i, float(u), float(thr)) for (l, i), u in zip(sel, iou)])
        cx, cy = (box[:, 0] + box[:, 2]) / 2.0, (box[:, 1] + box[:, 3]) / 2.0
        inside = torch.stack([cx - gt[g, 0], cy - gt[g, 1], gt[g, 2] - cx, gt[g, 3] - cy], 1).min(1)[0] > 0.01
        for (l, i), u, ok in zip(sel, iou, (iou >= thr) & inside):
            m = int(start[l]) + i
            if ok and u > best_iou[m]:                    # highest IoU; equal IoUs keep the lower box index
                best_iou[m], aidx[m], labels[m], targets[m] = u, g, gl[g], gt[g]
    return labels, aidx, weight, targets, cands


def assign(sizes, gts, gls, pad_shapes, topk=9, anchor_scale=8.0, num_classes=80, strides=STRIDES):
    """The batch, level-major: dict(labels, assign_idx, cls_weight, targets, npos [n], num_total = sum_i max(npos_i, 1))."""
    per = [assign_image(sizes, g, l, p, topk, anchor_scale, num_classes, strides)[:4] for g, l, p in zip(gts, gls, pad_shapes)]
    split = [h * w for h, w in sizes]
    out = []
    for k in range(4):
        parts = [t[k].split(split) for t in per]
        out.append(torch.cat([parts[i][l] for l in range(len(sizes)) for i in range(len(per))]))
    npos = [int((t[0] < num_classes).sum()) for t in per]
    return dict(labels=out[0], assign_idx=out[1], cls_weight=out[2], targets=out[3], npos=npos, num_total=sum(max(n, 1) for n in npos))


def flat_anchors(sizes, n, anchor_scale=8.0, strides=STRIDES):
    """[M, 4] anchors in level-major order for n images."""
    return torch.cat([a.repeat(n, 1) for a in level_anchors(sizes, anchor_scale, strides)])


def decode(anchors, deltas, stds=STDS, max_shape=None):
    """delta2bbox (means 0) in the dtype of `deltas`."""
    a = anchors.to(deltas.dtype)
    d = deltas * deltas.new_tensor(stds)
    px, py = (a[:, 0] + a[:, 2]) * 0.5, (a[:, 1] + a[:, 3]) * 0.5
    pw, ph = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    gw, gh = pw * d[:, 2].clamp(-MAX_RATIO, MAX_RATIO).exp(), ph * d[:, 3].clamp(-MAX_RATIO, MAX_RATIO).exp()
    gx, gy = px + pw * d[:, 0], py + ph * d[:, 1]
    b = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], 1)
    if max_shape is not None:
        H, W = float(max_shape[0]), float(max_shape[1])
        b = torch.stack([b[:, 0].clamp(0, W), b[:, 1].clamp(0, H), b[:, 2].clamp(0, W), b[:, 3].clamp(0, H)], 1)
    return b


def centerness_target(anchors, boxes):
    cx, cy = (anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2
    lr = torch.stack([cx - boxes[:, 0], boxes[:, 2] - cx], 1)
    tb = torch.stack([cy - boxes[:, 1], boxes[:, 3] - cy], 1)
    return ((lr.min(1)[0] / lr.max(1)[0]) * (tb.min(1)[0] / tb.max(1)[0])).sqrt()


def giou(p, t, eps=1e-6):
    a1, a2 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    wh = (torch.min(p[:, 2:], t[:, 2:]) - torch.max(p[:, :2], t[:, :2])).clamp(min=0)
    ov = wh[:, 0] * wh[:, 1]
    union = torch.max(a1 + a2 - ov, ov.new_tensor(eps))
    ewh = (torch.max(p[:, 2:], t[:, 2:]) - torch.min(p[:, :2], t[:, :2])).clamp(min=0)
    enc = torch.max(ewh[:, 0] * ewh[:, 1], ov.new_tensor(eps))
    return ov / union - (enc - union) / enc


def loss(cls, raw, ctr, scales, asg, sizes, n, num_classes=80, anchor_scale=8.0, stds=STDS, bbox_weight=1.0, cls_weight=1.0,
         ctr_weight=1.0, gamma=2.0, alpha=0.25, world=1.0, norm=None, strides=STRIDES):
    """float64 losses of flat level-major head outputs: cls [M, C], raw [M, 4] (the box predictor's output, in front of Scale), ctr [M],
    scales [5]; `asg` from assign().  norm = (sum of num_total over ranks, sum of centerness-target sums over ranks), default this
    rank's.  Returns (loss_cls, loss_bbox, loss_centerness) as graph-connected float64 scalars, and the centerness-target sum."""
    labels, weight, tgt = asg['labels'], asg['cls_weight'].double(), asg['targets'].double()
    lvl = torch.cat([torch.full((n * h * w,), i) for i, (h, w) in enumerate(sizes)])
    anchors = flat_anchors(sizes, n, anchor_scale, strides).double()
    pos = (labels < num_classes).nonzero().view(-1)
    ct = centerness_target(anchors[pos], tgt[pos]) if len(pos) else torch.zeros(0, dtype=torch.float64)
    tot, csum = (float(asg['num_total']), float(ct.sum())) if norm is None else norm
    num = max(tot / world, 1.0)
    den = max(csum / world, 1.0)
    x = cls.double()
    onehot = torch.zeros_like(x)
    onehot[pos, labels[pos]] = 1.0
    p = x.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    fw = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction='none')
    l_cls = (bce * fw * weight[:, None]).sum() / num * cls_weight
    if len(pos) == 0:
        return l_cls, raw.double().sum() * 0, ctr.double().sum() * 0, 0.0
    deltas = raw.double()[pos] * scales.double()[lvl[pos]][:, None]
    pred = decode(anchors[pos], deltas, stds)
    l_box = ((1 - giou(pred, tgt[pos])) * ct).sum() / den * bbox_weight
    l_ctr = torch.nn.functional.binary_cross_entropy_with_logits(ctr.double()[pos], ct, reduction='sum') / num * ctr_weight
    return l_cls, l_box, l_ctr, float(ct.sum())


def levels_to_flat(xs):
    """list of [n, K, h, w] -> [M, K] level-major."""
    return torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in xs])


def collect(cls, raw, ctr, scales, img_shape, scale_factor, flip_direction, nms_pre, anchor_scale=8.0, stds=STDS, strides=STRIDES):
    """aug_ref.collect with the ATSS decode: one view ([1, ., h, w] per level) -> mapped-back boxes [R, 4], scores [R, C], centerness [R]."""
    boxes, scores, cens = [], [], []
    H, W = float(img_shape[0]), float(img_shape[1])
    sizes = [tuple(c.shape[2:]) for c in cls]
    for l, (c, r, t, a) in enumerate(zip(cls, raw, ctr, level_anchors(sizes, anchor_scale, strides))):
        P = a.shape[0]
        sc = c[0].permute(1, 2, 0).reshape(P, -1).sigmoid()
        ce = t[0].reshape(P).sigmoid()
        x = r[0].permute(1, 2, 0).reshape(P, 4) * scales[l]
        if 0 < nms_pre < P:
            idx = (sc * ce[:, None]).max(1)[0].sort(descending=True, stable=True)[1][:nms_pre].sort()[0]
            sc, ce, x, a = sc[idx], ce[idx], x[idx], a[idx]
        boxes.append(decode(a, x, stds, (H, W)))
        scores.append(sc)
        cens.append(ce)
    b = torch.cat(boxes)
    if flip_direction in ('horizontal', 'diagonal'):
        b = torch.stack([W - b[:, 2], b[:, 1], W - b[:, 0], b[:, 3]], 1)
    if flip_direction in ('vertical', 'diagonal'):
        b = torch.stack([b[:, 0], H - b[:, 3], b[:, 2], H - b[:, 1]], 1)
    return b / torch.tensor(np.asarray(scale_factor, np.float32)), torch.cat(scores), torch.cat(cens)


def detect(cls, raw, ctr, scales, img_shapes, nms_pre=1000, score_thr=0.05, iou_thr=0.6, max_per_img=100, **kw):
    """Per image (dets [k, 5], labels [k]) through aug_ref.finish (detect_ref's rules), no rescale."""
    out = []
    for i in range(cls[0].shape[0]):
        view = [[x[i:i + 1] for x in t] for t in (cls, raw, ctr)]
        b, s, c = collect(*view, scales, img_shapes[i], np.ones(4, np.float32), None, nms_pre, **kw)
        out.append(A.finish(b, s, c, score_thr=score_thr, iou_thr=iou_thr, max_per_img=max_per_img, cap=16384)[:2])
    return out
