"""CPU model of the Fovea head as include/dsl_hip.h states it (no reference files are read here): the painted-rectangle assignment
in numpy float32 - operation by operation in the header's order - the focal + SmoothL1 loss in the dtype of its inputs (float64 with
autograd in the tests), and detection by way of tests/aug_ref.py's finish after the head's own decode.

Everything is level-major [level][image][y][x], as the kernels' buffers are.  test_fovea_cpu.py pins this model to the fixtures
tests/golden/fovea_*.npz, which hold what the reference's own FoveaHead computed."""
import numpy as np
import torch

import aug_ref as A
import loss_family_ref as LF

STRIDES = (8, 16, 32, 64, 128)
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
BASE = (16, 32, 64, 128, 256)
RANGES = ((1, 64), (32, 128), (64, 256), (128, 512), (256, 2048))      # configs/foveabox
F = np.float32


def flat_points(sizes, n, strides=STRIDES):
    """[M, 2] points (s (x + 0.5), s (y + 0.5)), [M] level and [M] image of every location, level-major for n images."""
    pts, lvl, img = [], [], []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        p = np.stack([(xs.reshape(-1) + 0.5) * s, (ys.reshape(-1) + 0.5) * s], 1)
        pts.append(np.tile(p, (n, 1)))
        lvl.append(np.full(n * h * w, l))
        img.append(np.repeat(np.arange(n), h * w))
    return np.concatenate(pts).astype(np.float32), np.concatenate(lvl), np.concatenate(img)


def fovea_rect(box, s, sigma, h, w):
    """(left, right, top, down) of one box on a level after the clamp, in fp32 as the kernel computes them."""
    b = box.astype(F) / F(s)
    hw, hh = F(0.5) * (b[2] - b[0]), F(0.5) * (b[3] - b[1])
    oms, ops = F(1.0 - float(F(sigma))), F(1.0 + float(F(sigma)))
    half = F(0.5)
    left = min(max(np.ceil(b[0] + oms * hw - half), 0), w - 1)
    right = min(max(np.floor(b[0] + ops * hw - half), 0), w - 1)
    top = min(max(np.ceil(b[1] + oms * hh - half), 0), h - 1)
    down = min(max(np.floor(b[1] + ops * hh - half), 0), h - 1)
    return int(left), int(right), int(top), int(down)


def assign(gts, gls, sizes, num_classes, sigma=0.4, base=BASE, ranges=RANGES, strides=STRIDES):
    """gts / gls: per image [G, 4] / [G].  Returns labels (int64), assign_idx (int32, box index in the image, -1 = none), targets
    ([M, 4] log targets, exactly 0 where nothing was painted), cls_weight, pos_weight, num_pos and stats[0:2]."""
    n = len(gts)
    labels, idxs, tgts = [], [], []
    for (h, w), s, bl, (lo, hi) in zip(sizes, strides, base, ranges):
        for i in range(n):
            gt = np.asarray(gts[i], F).reshape(-1, 4)
            gl = np.asarray(gls[i]).reshape(-1)
            area = np.sqrt((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))
            lab = np.full((h, w), num_classes, np.int64)
            idx = np.full((h, w), -1, np.int32)
            raw = np.ones((h, w, 4), F)
            with np.errstate(invalid='ignore'):
                hit = np.nonzero((area >= F(lo)) & (area <= F(hi)))[0]
            # decreasing area; equal areas: ascending index, so that the higher index is painted last (the kernel's rule)
            for g in hit[np.argsort(-area[hit], kind='stable')]:
                left, right, top, down = fovea_rect(gt[g], s, sigma, h, w)
                if left > right or top > down:
                    continue
                px = (F(s) * (np.arange(left, right + 1).astype(F) + F(0.5)))[None, :]
                py = (F(s) * (np.arange(top, down + 1).astype(F) + F(0.5)))[:, None]
                lab[top:down + 1, left:right + 1] = gl[g]
                idx[top:down + 1, left:right + 1] = g
                cell = raw[top:down + 1, left:right + 1]
                cell[..., 0] = (px - gt[g, 0]) / F(bl)
                cell[..., 1] = (py - gt[g, 1]) / F(bl)
                cell[..., 2] = (gt[g, 2] - px) / F(bl)
                cell[..., 3] = (gt[g, 3] - py) / F(bl)
            t = np.log(np.clip(raw, F(1.0 / 16.0), F(16.0))).astype(F)
            t[idx < 0] = 0
            labels.append(lab.reshape(-1))
            idxs.append(idx.reshape(-1))
            tgts.append(t.reshape(-1, 4))
    labels, idxs, tgts = np.concatenate(labels), np.concatenate(idxs), np.concatenate(tgts)
    num_pos = int((labels < num_classes).sum())
    M = len(labels)
    return dict(labels=torch.from_numpy(labels), assign_idx=torch.from_numpy(idxs), targets=torch.from_numpy(tgts),
                cls_weight=torch.ones(M), pos_weight=torch.ones(M), num_pos=num_pos,
                stats=(float(num_pos + n), float(max(num_pos, 1))))


def smooth_l1(d, beta):
    a = d.abs()
    return torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta)


def loss(cls, raw, asg, n, num_classes, gamma=2.0, alpha=0.25, beta=0.11, cls_weight=1.0, bbox_weight=1.0):
    """cls [M, C] logits, raw [M, 4] conv_reg outputs, `asg` from assign().  Returns (loss_cls, loss_bbox), graph-connected."""
    labels = asg['labels']
    num_pos = int((labels < num_classes).sum())
    l_cls = LF.focal_loss_elem(cls, labels, num_classes, gamma, alpha).sum() / float(num_pos + n) * cls_weight
    pos = (labels < num_classes).nonzero().view(-1)
    if len(pos) == 0:
        return l_cls, raw.sum() * 0
    l_box = smooth_l1(raw[pos] - asg['targets'][pos].to(raw.dtype), beta).sum() / float(num_pos) * bbox_weight
    return l_cls, l_box


def collect(cls, raw, img_shape, scale_factor, nms_pre, base=BASE, strides=STRIDES):
    """One image ([1, C|4, h, w] per level) -> boxes [R, 4] (divided by scale_factor), scores [R, C], a unit centerness [R]."""
    boxes, scores = [], []
    H, W = float(img_shape[0]), float(img_shape[1])
    for c, r, s, bl in zip(cls, raw, strides, base):
        h, w = c.shape[2:]
        P = h * w
        sc = c[0].permute(1, 2, 0).reshape(P, -1).sigmoid()
        d = r[0].permute(1, 2, 0).reshape(P, 4).exp() * bl
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        px, py = ((xs.reshape(-1) + 0.5) * s).to(d.dtype), ((ys.reshape(-1) + 0.5) * s).to(d.dtype)
        if 0 < nms_pre < P:      # (equal keys: the lowest indices, the kernels' rule)
            idx = sc.max(1)[0].sort(descending=True, stable=True)[1][:nms_pre].sort()[0]
            sc, d, px, py = sc[idx], d[idx], px[idx], py[idx]
        boxes.append(torch.stack([(px - d[:, 0]).clamp(0, W - 1), (py - d[:, 1]).clamp(0, H - 1), (px + d[:, 2]).clamp(0, W - 1),
                                  (py + d[:, 3]).clamp(0, H - 1)], 1))
        scores.append(sc)
    s = torch.cat(scores)
    return torch.cat(boxes) / torch.from_numpy(np.array(scale_factor, np.float64)).to(boxes[0].dtype), s, torch.ones(s.shape[0], dtype=s.dtype)


def detect(cls, raw, img_shapes, scale_factors=None, nms_pre=1000, score_thr=0.05, iou_thr=0.5, max_per_img=100, base=BASE):
    """Per image (dets [k, 5], labels [k]) through aug_ref.finish (the project's CPU NMS model); scale_factors None: no rescale."""
    out = []
    for i in range(cls[0].shape[0]):
        sf = np.ones(4) if scale_factors is None else np.broadcast_to(np.asarray(scale_factors[i], np.float64).reshape(-1), (4,))
        b, s, c = collect([x[i:i + 1] for x in cls], [x[i:i + 1] for x in raw], img_shapes[i], sf, nms_pre, base)
        out.append(A.finish(b, s, c, score_thr=score_thr, iou_thr=iou_thr, max_per_img=max_per_img, cap=16384)[:2])
    return out


def flat(ts):
    """Per-level [n, K, h, w] tensors -> [M, K] level-major."""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts])


def unflat(t, sizes, n):
    """[M, K] level-major -> per-level [n, K, h, w]."""
    out, o = [], 0
    for h, w in sizes:
        out.append(t[o:o + n * h * w].reshape(n, h, w, -1).permute(0, 3, 1, 2))
        o += n * h * w
    return out
