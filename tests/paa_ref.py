"""Numpy / torch (CPU) model of the PAA head as include/dsl_hip.h states it (no reference files and no sklearn are read here): the
MaxIoU first assignment in fp32 with its low-quality pass, the candidates' losses, the per-box top-k, the two-component Gaussian
mixture fit in float64 on the fp32 losses (its own EM loop), the separation scheme, the three losses in float64 with autograd, and
detection with sqrt(cls * iou) scores and score voting.

Everything is level-major [level][image][y][x], as the kernels' buffers are.  test_paa_cpu.py pins this model to the fixtures
tests/golden/paa_*.npz, which hold what the reference's own PAAHead (with sklearn's GaussianMixture) computed."""
import math

import numpy as np
import torch

import atss_ref as AR

STRIDES, SIZES, STDS = AR.STRIDES, AR.SIZES, AR.STDS
TOL, REG_COVAR, MAX_ITER = 1e-3, 1e-6, 100
LOG_2PI_F32 = float(np.float32(math.log(2.0 * math.pi)))      # sklearn: np.log(2 * np.pi).astype(X.dtype), X float32
EPS_IOU = 1e-12                                                # paa_head.py:20, the clamp of loss_bbox's weight


def mstarts(sizes, n):
    return np.cumsum([0] + [n * h * w for h, w in sizes])


def assign_image(sizes, gt, gl, pad_shape, pos_iou_thr=0.1, anchor_scale=8.0, num_classes=80, strides=STRIDES):
    """MaxIoUAssigner(pos_iou_thr = neg_iou_thr, min_pos_iou = 0, gt_max_assign_all) on the valid anchors of one image, fp32.
    Returns labels, cand_gt (-1 = none), cls_weight, targets over the image's locations in level order."""
    anchors, valid = torch.cat(AR.level_anchors(sizes, anchor_scale, strides)), torch.cat(AR.valid_masks(sizes, pad_shape, strides))
    P = anchors.shape[0]
    labels = torch.full((P,), num_classes, dtype=torch.long)
    cand = torch.full((P,), -1, dtype=torch.int32)
    targets = torch.zeros(P, 4)
    gt = gt.reshape(-1, 4).float()
    if gt.shape[0]:
        iou = AR.iou_matrix(anchors, gt)                       # [P, G]
        iou[~valid] = -1.0                                     # an invalid anchor takes no part
        best = iou.max(1)[0]
        first = (iou == best[:, None]).int().argmax(1).int()     # equal maxima: the lower box index
        hit = valid & (best >= np.float32(pos_iou_thr))
        cand[hit] = first[hit]
        gmax = iou.max(0)[0]
        for g in range(gt.shape[0]):                            # the low-quality pass: a later box overwrites an earlier one
            hit = valid & (iou[:, g] == gmax[g])
            cand[hit] = g
        pos = cand >= 0
        labels[pos] = gl[cand[pos].long()]
        targets[pos] = gt[cand[pos].long()]
    return labels, cand, valid.float(), targets


def assign(sizes, gts, gls, pad_shapes, pos_iou_thr=0.1, anchor_scale=8.0, num_classes=80, strides=STRIDES):
    per = [assign_image(sizes, g, l, p, pos_iou_thr, anchor_scale, num_classes, strides) for g, l, p in zip(gts, gls, pad_shapes)]
    split = [h * w for h, w in sizes]
    out = []
    for k in range(4):
        parts = [t[k].split(split) for t in per]
        out.append(torch.cat([parts[i][l] for l in range(len(sizes)) for i in range(len(per))]))
    return dict(labels=out[0], cand_gt=out[1], cls_weight=out[2], targets=out[3])


def focal_terms(x, onehot, gamma=2.0, alpha=0.25):
    p = x.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    fw = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    return torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction='none') * fw


def levels_of(sizes, n):
    return torch.cat([torch.full((n * h * w,), i) for i, (h, w) in enumerate(sizes)])


def decoded(raw, scales, idx, sizes, n, anchor_scale, stds, strides=STRIDES, dtype=torch.float64):
    lvl = levels_of(sizes, n)
    anchors = AR.flat_anchors(sizes, n, anchor_scale, strides).to(dtype)
    return AR.decode(anchors[idx], raw.to(dtype)[idx] * scales.to(dtype)[lvl[idx]][:, None], stds)


def pos_loss(cls, raw, scales, asg, sizes, n, num_classes=80, anchor_scale=8.0, stds=STDS, bbox_weight=1.0, cls_weight=1.0,
             gamma=2.0, alpha=0.25, strides=STRIDES, dtype=torch.float64):
    """[M]: w_cls * sum_c focal + w_bbox * (1 - GIoU(decode, target)) for every candidate, 0 elsewhere."""
    idx = (asg['cand_gt'] >= 0).nonzero().view(-1)
    out = torch.zeros(cls.shape[0], dtype=dtype)
    if len(idx) == 0:
        return out
    x = cls.to(dtype)[idx]
    onehot = torch.zeros_like(x)
    onehot[torch.arange(len(idx)), asg['labels'][idx]] = 1.0
    pred = decoded(raw, scales, idx, sizes, n, anchor_scale, stds, strides, dtype)
    out[idx] = cls_weight * focal_terms(x, onehot, gamma, alpha).sum(1) + bbox_weight * (1 - AR.giou(pred, asg['targets'].to(dtype)[idx]))
    return out


def _logsumexp2(a, b):
    m = np.maximum(a, b)
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def gmm_fit(x32):
    """GaussianMixture(2, 'diag', weights (0.5, 0.5), means (min, max), precisions (1, 1)).fit on the float32 column x32, restated in
    float64: the samples stay float32 (x * x and the first iteration's mean^2 are float32 products), log(2 pi) is rounded to float32.
    Returns dict(flag 0 fitted | 2 non-positive variance, n_iter, pred, scores, stop / pred / gap margins, var_margin = the smallest
    |variance| of any iteration: how far every variance stayed from the sign test)."""
    x32 = np.asarray(x32, np.float32)
    x, xx = x32.astype(np.float64), (x32 * x32).astype(np.float64)
    n = len(x)
    w = np.array([0.5, 0.5])
    mu = np.array([x32.min(), x32.max()], np.float64)
    mu2 = (np.array([x32.min(), x32.max()], np.float32) ** 2).astype(np.float64)
    pc = np.array([1.0, 1.0])

    def wlp(mu, mu2, pc, w):
        prec = pc ** 2
        lp = mu2[None] * prec[None] - 2.0 * (x[:, None] * (mu * prec)[None]) + xx[:, None] * prec[None]
        return -0.5 * (LOG_2PI_F32 + lp) + np.log(pc)[None] + np.log(w)[None]

    lower, stop_margin, var_margin, it = -np.inf, np.inf, np.inf, 0
    for it in range(1, MAX_ITER + 1):
        prev = lower
        a = wlp(mu, mu2, pc, w)
        norm = _logsumexp2(a[:, 0], a[:, 1])
        resp = np.exp(a - norm[:, None])
        nk = resp.sum(0) + 10 * np.finfo(np.float64).eps
        mu = (resp * x[:, None]).sum(0) / nk
        mu2 = mu ** 2
        var = (resp * xx[:, None]).sum(0) / nk - mu2 + REG_COVAR
        w = nk / nk.sum()
        var_margin = min(var_margin, float(np.abs(var).min()))
        if np.any(var <= 0.0):
            return dict(flag=2, n_iter=it, stop_margin=float(stop_margin), var_margin=var_margin)
        pc = 1.0 / np.sqrt(var)
        lower = norm.mean()
        change = lower - prev
        stop_margin = min(stop_margin, abs(abs(change) - TOL))
        if abs(change) < TOL:
            break
    a = wlp(mu, mu2, pc, w)
    pred = (a[:, 1] > a[:, 0]).astype(np.int64)
    scores = _logsumexp2(a[:, 0], a[:, 1])
    fg = scores[pred == 0]
    srt = np.sort(fg)[::-1]
    return dict(flag=0, n_iter=it, pred=pred, scores=scores, stop_margin=float(stop_margin), var_margin=var_margin,
                pred_margin=float(np.abs(a[:, 0] - a[:, 1]).min()), gap=float(srt[0] - srt[1]) if len(srt) > 1 else np.inf)


def reassign(ploss, asg, sizes, n, gt_counts, topk=9, num_classes=80):
    """ploss: float32 [M].  TIE RULE: equal losses go to the lower anchor index.  Returns dict(labels, kept [M] bool, npos [n],
    boxes = per (image, box) dict(samples, index, flag, n_iter, pred, scores, npos))."""
    ploss = np.asarray(ploss, np.float32)
    cand = asg['cand_gt'].numpy()
    ms = mstarts(sizes, n)
    kept = np.zeros(len(cand), bool)
    boxes, npos = [], [0] * n
    for i in range(n):
        for g in range(gt_counts[i]):
            sel = []
            for l, (h, w) in enumerate(sizes):
                lo = ms[l] + i * h * w
                idx = lo + (cand[lo:lo + h * w] == g).nonzero()[0]
                order = np.lexsort((idx, ploss[idx]))[:min(topk, len(idx))]
                sel.append(idx[order])
            sel = np.concatenate(sel)
            sel = sel[np.lexsort((sel, ploss[sel]))]
            rec = dict(image=i, box=g, index=sel, samples=ploss[sel], flag=0, n_iter=0, npos=0)
            if len(sel) < 2:
                rec['flag'] = 1
            else:
                rec.update(gmm_fit(ploss[sel]))
                if rec['flag'] == 0:
                    fg = (rec['pred'] == 0).nonzero()[0]
                    if len(fg):
                        j = int(np.argmax(rec['scores'][fg]))
                        kept[sel[fg[:j + 1]]] = True
                        rec['npos'] = j + 1
            npos[i] += rec['npos']
            boxes.append(rec)
    labels = asg['labels'].clone()
    labels[torch.from_numpy(~kept)] = num_classes
    return dict(labels=labels, kept=torch.from_numpy(kept), npos=npos, boxes=boxes)


def iou_targets(raw, scales, asg, re, sizes, n, anchor_scale=8.0, stds=STDS, strides=STRIDES, dtype=torch.float64):
    """[M]: aligned bbox_overlaps(decode, target), union clamped at 1e-6, for the kept anchors; 0 elsewhere."""
    out = torch.zeros(raw.shape[0], dtype=dtype)
    pos = re['kept'].nonzero().view(-1)
    if len(pos):
        p, t = decoded(raw, scales, pos, sizes, n, anchor_scale, stds, strides, dtype), asg['targets'].to(dtype)[pos]
        wh = (torch.min(p[:, 2:], t[:, 2:]) - torch.max(p[:, :2], t[:, :2])).clamp(min=0)
        ov = wh[:, 0] * wh[:, 1]
        a1, a2 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
        out[pos] = ov / torch.max(a1 + a2 - ov, ov.new_tensor(1e-6))
    return out


def loss(cls, raw, iou_logit, scales, asg, re, sizes, n, num_classes=80, anchor_scale=8.0, stds=STDS, bbox_weight=1.0, cls_weight=1.0,
         iou_weight=1.0, gamma=2.0, alpha=0.25, strides=STRIDES):
    """float64 losses (paa_head.py:169-199) of flat level-major head outputs; returns (loss_cls, loss_bbox, loss_iou), graph-connected,
    and the IoU targets [M]."""
    labels, weight = re['labels'], asg['cls_weight'].double()
    pos = re['kept'].nonzero().view(-1)
    num_pos = float(sum(re['npos']))
    x = cls.double()
    onehot = torch.zeros_like(x)
    onehot[pos, labels[pos]] = 1.0
    l_cls = (focal_terms(x, onehot, gamma, alpha) * weight[:, None]).sum() / max(num_pos, float(n)) * cls_weight
    if len(pos) == 0:
        return l_cls, raw.double().sum() * 0, iou_logit.double().sum() * 0, torch.zeros(raw.shape[0], dtype=torch.float64)
    pred = decoded(raw, scales, pos, sizes, n, anchor_scale, stds, strides)
    tgt = asg['targets'].double()[pos]
    it = iou_targets(raw.detach(), scales.detach(), asg, re, sizes, n, anchor_scale, stds, strides)
    l_iou = torch.nn.functional.binary_cross_entropy_with_logits(iou_logit.double()[pos], it[pos], reduction='sum') / num_pos * iou_weight
    l_box = ((1 - AR.giou(pred, tgt)) * it[pos].clamp(min=EPS_IOU)).sum() / it[pos].sum() * bbox_weight
    return l_cls, l_box, l_iou, it


# ---- detection --------------------------------------------------------------------------------------------------------------------
def _nms(boxes, scores, thr, compared=None):
    """Greedy NMS on class-offset boxes; compared (a list): takes the IoUs of the comparisons that decide (kept box against every
    candidate still in the running)."""
    order = np.argsort(-scores, kind='stable')
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    sup, keep = np.zeros(len(boxes), bool), []
    for i in order:
        if sup[i]:
            continue
        keep.append(i)
        wh = np.clip(np.minimum(boxes[i, 2:], boxes[:, 2:]) - np.maximum(boxes[i, :2], boxes[:, :2]), 0, None)
        inter = wh[:, 0] * wh[:, 1]
        with np.errstate(invalid='ignore'):
            iou = inter / (area[i] + area - inter)
        if compared is not None:
            compared.append(iou[~sup & (inter > 0)])
        sup |= iou > thr
    return np.asarray(keep, np.int64)


def detect_image(cls, raw, iou, scales, img_shape, scale_factor, nms_pre=1000, score_thr=0.05, iou_thr=0.6, max_per_img=100,
                 score_voting=True, anchor_scale=8.0, stds=STDS, strides=STRIDES, vote_dtype=np.float64, compared=None):
    """One image ([C, h, w] / [4, h, w] / [1, h, w] per level), rescale=True.  The candidates, the NMS and the scores are fp32 as the
    kernels'; the vote runs in vote_dtype.  Returns dets [k, 5] (class ascending, then NMS order, when voting; else NMS order),
    labels [k], and the unvoted boxes in the same order."""
    H, W = float(img_shape[0]), float(img_shape[1])
    sizes = [tuple(c.shape[1:]) for c in cls]
    bs, ss = [], []
    for l, (c, r, t, a) in enumerate(zip(cls, raw, iou, AR.level_anchors(sizes, anchor_scale, strides))):
        P = a.shape[0]
        sc = (c.permute(1, 2, 0).reshape(P, -1).sigmoid() * t.reshape(P).sigmoid()[:, None]).sqrt()
        x = r.permute(1, 2, 0).reshape(P, 4) * scales[l]
        if 0 < nms_pre < P:
            idx = sc.max(1)[0].sort(descending=True, stable=True)[1][:nms_pre].sort()[0]
            sc, x, a = sc[idx], x[idx], a[idx]
        bs.append(AR.decode(a, x, stds, (H, W)))
        ss.append(sc)
    boxes = (torch.cat(bs) / torch.tensor(np.asarray(scale_factor, np.float32))).numpy()
    scores = torch.cat(ss).numpy()
    pi, pc = np.nonzero(scores > np.float32(score_thr))
    pb, ps = boxes[pi], scores[pi, pc]
    if len(pb) == 0:
        return np.zeros((0, 5), np.float32), np.zeros(0, np.int64), np.zeros((0, 4), np.float32)
    off = pc.astype(np.float32) * (pb.max() + np.float32(1))
    keep = _nms(pb + off[:, None], ps, iou_thr, compared)[:max_per_img]
    kb, ks, kl = pb[keep], ps[keep], pc[keep]
    if not score_voting:
        return np.concatenate([kb, ks[:, None]], 1), kl, kb
    order = np.argsort(kl, kind='stable')
    kb, ks, kl = kb[order], ks[order], kl[order]
    out = np.zeros((len(kb), 5), np.float32)
    for k in range(len(kb)):
        m = pc == kl[k]
        cb, cs = pb[m].astype(vote_dtype), ps[m].astype(vote_dtype)
        d = kb[k].astype(vote_dtype)
        wh = np.clip(np.minimum(d[2:], cb[:, 2:]) - np.maximum(d[:2], cb[:, :2]), 0, None)
        ov = wh[:, 0] * wh[:, 1]
        union = np.maximum((d[2] - d[0]) * (d[3] - d[1]) + (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1]) - ov, vote_dtype(1e-6))
        io = ov / union
        sel = io > 0.01
        p = np.exp(-(1 - io[sel]) ** 2 / 0.025) * cs[sel]
        out[k, :4] = (p[:, None] * cb[sel]).sum(0) / p.sum()
        out[k, 4] = ks[k]
    return out, kl, kb
