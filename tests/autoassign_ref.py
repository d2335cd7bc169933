"""CPU model of the AutoAssign head as include/dsl_hip.h states it (no reference files are read here): points, decode, inside mask,
centre prior, the per-point maximum IoU, the negative weights with their same-class rule and the three losses, in the dtype of its
inputs (float64 with autograd in the tests; float32 to show what fp32 itself holds).

Everything is level-major [level][image][y][x], as the kernels' buffers are.  test_autoassign_cpu.py pins this model to the fixtures
tests/golden/autoassign_*.npz, which hold what the reference's own AutoAssignHead computed."""
import numpy as np
import torch

STRIDES = (8, 16, 32, 64, 128)
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
EPS = 1e-12


def flat_points(sizes, n, strides=STRIDES):
    """[M, 2] points (s x, s y) - no half-stride offset - [M] level and [M] image of every location, level-major for n images."""
    pts, lvl, img = [], [], []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        p = np.stack([xs.reshape(-1) * s, ys.reshape(-1) * s], 1)
        pts.append(np.tile(p, (n, 1)))
        lvl.append(np.full(n * h * w, l))
        img.append(np.repeat(np.arange(n), h * w))
    return np.concatenate(pts).astype(np.float64), np.concatenate(lvl), np.concatenate(img)


def decode(raw, scales, pts, lvl, strides=STRIDES):
    """bbox_pred = relu(scale_l x) s_l and the decoded box (px - l, py - t, px + r, py + b)."""
    s = torch.as_tensor(np.asarray(strides, np.float64)[lvl], dtype=raw.dtype)
    d = torch.relu(raw * scales[torch.as_tensor(lvl)][:, None]) * s[:, None]
    p = torch.as_tensor(pts, dtype=raw.dtype)
    return d, torch.stack([p[:, 0] - d[:, 0], p[:, 1] - d[:, 1], p[:, 0] + d[:, 2], p[:, 1] + d[:, 3]], 1)


def inside_mask(pts, gt):
    """[P, G] bool: min(l, t, r, b) > 0, in the boxes' own fp32."""
    p = np.asarray(pts, np.float32)
    g = np.asarray(gt, np.float32).reshape(-1, 4)
    m = np.minimum(np.minimum(p[:, None, 0] - g[None, :, 0], p[:, None, 1] - g[None, :, 1]),
                   np.minimum(g[None, :, 2] - p[:, None, 0], g[None, :, 3] - p[:, None, 1]))
    return torch.from_numpy(m > 0)


def center_prior(pts, stride, gt, gl, mean, sigma, inside):
    """c(i, g) = prod_d exp(-(((p_d - centre_d) / s - mean[label, d])^2) / (2 sigma[label, d]^2)) at inside pairs, else 0."""
    dt = mean.dtype
    p, s, g = torch.as_tensor(pts, dtype=dt), torch.as_tensor(stride, dtype=dt), gt.to(dt)
    ctr = torch.stack([(g[:, 0] + g[:, 2]) / 2, (g[:, 1] + g[:, 3]) / 2], 1)
    dist = ((p[:, None, :] - ctr[None]) / s[:, None, None] - mean[gl][None]) ** 2
    c = torch.exp(-dist / (2 * sigma[gl][None] ** 2)).prod(-1)
    return torch.where(inside, c, torch.zeros_like(c))


def pair_iou(a, b, giou=False, eps=1e-6):
    """a [P, 4] against b [G, 4] -> [P, G]: bbox_overlaps (mode 'iou' / 'giou', eps on union and enclosing area)."""
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    ov = wh[..., 0] * wh[..., 1]
    un = (a1[:, None] + a2[None] - ov).clamp(min=eps)
    iou = ov / un
    if not giou:
        return iou
    elt = torch.min(a[:, None, :2], b[None, :, :2])
    erb = torch.max(a[:, None, 2:], b[None, :, 2:])
    ewh = (erb - elt).clamp(min=0)
    en = (ewh[..., 0] * ewh[..., 1]).clamp(min=eps)
    return iou - (en - un) / en


def neg_weight(iou, inside, gl, C):
    """p_neg_weight [P, C]: boxes in ascending index, so the highest index of a class wins a shared point."""
    w = torch.ones(iou.shape[0], C, dtype=iou.dtype)
    for g in range(inside.shape[1]):
        m = inside[:, g]
        if bool(m.any()):
            t = 1 / (1 - iou[m]).clamp(min=EPS)
            w[m, int(gl[g])] = 1 - (t - t.min() + EPS) / (t.max() - t.min() + EPS)
    return w


def loss(cls, raw, obj, scales, mean, sigma, gts, gls, sizes, num_classes, pos_w=0.25, neg_w=0.75, center_w=0.75, bbox_weight=5.0,
         strides=STRIDES, world=None):
    """cls [M, C] logits, raw [M, 4] conv_reg outputs, obj [M] objectness logits.  Returns a dict: loss_pos / loss_neg / loss_center
    (graph-connected), stats (box count, sum c: this rank's), and per image inside / prior / iou / negw.  `world`: (sum of the ranks'
    box counts, sum of their sum c, 1 / world_size) for the two reduce_mean normalisers; None = this rank alone."""
    n = len(gts)
    pts, lvl, img = flat_points(sizes, n, strides)
    dt = cls.dtype
    dist, box = decode(raw, scales, pts, lvl, strides)
    pc, po = cls.sigmoid(), obj.reshape(-1).sigmoid()
    out = dict(inside=[], prior=[], iou=[], negw=[], R=[])
    nbox = sum(len(g) for g in gts)
    pos_sum = cls.sum() * 0
    neg_sum = cls.sum() * 0
    center, csum = [], 0.0
    st = np.asarray(strides, np.float64)[lvl]
    for i in range(n):
        idx = torch.as_tensor(np.nonzero(img == i)[0])
        gt, gl = torch.as_tensor(np.asarray(gts[i], np.float32).reshape(-1, 4)), torch.as_tensor(np.asarray(gls[i]).reshape(-1)).long()
        G = len(gl)
        ins = inside_mask(pts[idx], gt)
        c = center_prior(pts[idx], st[idx], gt, gl, mean, sigma, ins)
        pci, poi, bi = pc[idx], po[idx], box[idx]
        iou = torch.zeros(len(idx), dtype=dt)
        if G:
            with torch.no_grad():
                iou = pair_iou(bi, gt.to(dt)).max(1).values
            reg = bbox_weight * (1 - pair_iou(bi, gt.to(dt), giou=True))
            p_pos = pci[:, gl] * poi[:, None] * torch.exp(-reg)
            wgt = torch.exp(3 * p_pos) * c
            R = (p_pos * wgt).sum(0) / wgt.sum(0).clamp(min=EPS)
            pos_sum = pos_sum + torch.nn.functional.binary_cross_entropy(R, torch.ones_like(R), reduction='none').sum()
            out['R'].append(R.detach())
        else:
            out['R'].append(torch.zeros(0, dtype=dt))
        negw = neg_weight(iou.detach(), ins, gl, num_classes)
        q = pci * poi[:, None] * negw
        neg_sum = neg_sum + (q ** 2 * torch.nn.functional.binary_cross_entropy(q, torch.zeros_like(q), reduction='none')).sum()
        csum = csum + float(c.detach().sum())
        center.append(G / c.sum().clamp(min=EPS) if bool(ins.any()) else c.sum() * 0)
        out['inside'].append(ins); out['prior'].append(c.detach()); out['iou'].append(iou.detach()); out['negw'].append(negw)
    wb, wc, inv = (float(nbox), csum, 1.0) if world is None else world
    out['stats'] = (float(nbox), csum)
    out['loss_neg'] = neg_sum * neg_w / max(wc * inv, 1.0)
    if nbox == 0:      # (:433-437)
        out['loss_pos'] = raw.sum() * 0
        out['loss_center'] = obj.sum() * 0 + mean.sum() * 0 + sigma.sum() * 0
    else:
        out['loss_pos'] = pos_sum * pos_w / max(wb * inv, 1.0)
        out['loss_center'] = torch.stack(center).mean() * center_w
    return out


def collect(cls, raw, obj, scales, img_shape, scale_factor, nms_pre, flip_direction=None, strides=STRIDES):
    """One image or view ([1, C|4|1, h, w] per level) -> boxes [R, 4] (mapped back through the flip, divided by scale_factor), scores
    [R, C], objectness [R]: FCOSHead._get_bboxes (fcos_head.py:419-516) on the points (x s, y s) with relu(scale x) s."""
    boxes, scores, cens = [], [], []
    H, W = float(img_shape[0]), float(img_shape[1])
    for c, r, t, sc_l, s in zip(cls, raw, obj, scales, strides):
        h, w = c.shape[2:]
        P = h * w
        sc = c[0].permute(1, 2, 0).reshape(P, -1).sigmoid()
        ce = t[0].reshape(P).sigmoid()
        d = torch.relu(r[0].permute(1, 2, 0).reshape(P, 4) * sc_l) * s
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        px, py = (xs.reshape(-1) * s).to(d.dtype), (ys.reshape(-1) * s).to(d.dtype)
        if 0 < nms_pre < P:      # (equal keys: the lowest indices, the kernels' rule)
            idx = (sc * ce[:, None]).max(1)[0].sort(descending=True, stable=True)[1][:nms_pre].sort()[0]
            sc, ce, d, px, py = sc[idx], ce[idx], d[idx], px[idx], py[idx]
        boxes.append(torch.stack([(px - d[:, 0]).clamp(0, W), (py - d[:, 1]).clamp(0, H), (px + d[:, 2]).clamp(0, W), (py + d[:, 3]).clamp(0, H)], 1))
        scores.append(sc)
        cens.append(ce)
    b = torch.cat(boxes)
    if flip_direction in ('horizontal', 'diagonal'):
        b = torch.stack([W - b[:, 2], b[:, 1], W - b[:, 0], b[:, 3]], 1)
    if flip_direction in ('vertical', 'diagonal'):
        b = torch.stack([b[:, 0], H - b[:, 3], b[:, 2], H - b[:, 1]], 1)
    return b / torch.from_numpy(np.array(scale_factor, np.float64)).to(b.dtype), torch.cat(scores), torch.cat(cens)


def detect(cls, raw, obj, scales, img_shapes, scale_factors=None, nms_pre=1000, score_thr=0.05, iou_thr=0.6, max_per_img=100):
    """Per image (dets [k, 5], labels [k]) through aug_ref.finish (the project's CPU NMS model); scale_factors None: no rescale."""
    import aug_ref as A
    out = []
    for i in range(cls[0].shape[0]):
        sf = np.ones(4) if scale_factors is None else np.broadcast_to(np.asarray(scale_factors[i], np.float64).reshape(-1), (4,))
        b, s, c = collect([x[i:i + 1] for x in cls], [x[i:i + 1] for x in raw], [x[i:i + 1] for x in obj], scales, img_shapes[i], sf, nms_pre)
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


def image_rows(sizes, n, i):
    """The level-major rows of image i in the order of its P points (level, y, x): what the fixtures' per-image arrays index."""
    _, _, img = flat_points(sizes, n)
    return np.nonzero(img == i)[0]
