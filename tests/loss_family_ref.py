"""torch-CPU restatement of FCOSHead.loss (fcos_head.py:170-338) with the loss family: loss_bbox of kind giou / iou / iou_linear /
diou / ciou (losses/iou_loss.py:14-36, :85-219), FocalLoss gamma / alpha (losses/focal_loss.py:11-56) and the three loss_weights.

Targets, points, the centerness target, the aligned IoU / GIoU and the model around the loss come from tests/head_options_ref.py
and oracle/fcos_oracle.py.  Two deliberate deviations from the reference's fp32 arithmetic, the ones the kernel documents:
  * CIoU's penalty v^2 / (1 - iou + v) and its gradient are 0 where v == 0 (the reference: 0/0 = NaN when prediction and target
    coincide; 0 is the float64 value);
  * the focal gradient is the analytic -+alpha q^gamma (gamma p sp + q), finite where autograd's pow backward gives NaN (gamma < 1 with
    the sigmoid saturated to exactly 0 or 1).
tests/test_loss_family_cpu.py pins this file to the reference's own outputs (tests/golden/loss_fam_*.npz)."""
import math

import torch
import torch.nn.functional as F

import head_options_ref as HR
from oracle import fcos_oracle as O

DEFAULT_LOSS = dict(box_loss=None, box_eps=1e-6, focal_gamma=2.0, focal_alpha=0.25, cls_weight=1.0, bbox_weight=1.0, ctr_weight=1.0)


def loss_settings(**kw):
    s = dict(DEFAULT_LOSS)
    s.update(kw)
    return s


class _Focal(torch.autograd.Function):
    """focal_loss.py:34-40 per element; backward: d/dx = -alpha q^gamma (gamma p sp + q) for target 1, (1 - alpha) p^gamma (gamma q sp' + p)
    for target 0, with q = 1 - p, sp = -log p, sp' = -log(1 - p) - no q^(gamma - 1)."""

    @staticmethod
    def forward(ctx, x, t, gamma, alpha):
        p = x.sigmoid()
        q = (-x).sigmoid()
        pt = q * t + p * (1 - t)
        mod = pt.pow(gamma)                      # pow(0, 0) = 1
        bce = F.binary_cross_entropy_with_logits(x, t, reduction='none')
        ctx.save_for_backward(p, q, t, mod, bce)
        ctx.gamma, ctx.alpha = gamma, alpha
        return (alpha * t + (1 - alpha) * (1 - t)) * mod * bce

    @staticmethod
    def backward(ctx, g):
        p, q, t, mod, bce = ctx.saved_tensors
        gm, a = ctx.gamma, ctx.alpha
        d1 = -a * mod * (gm * p * bce + q)
        d0 = (1 - a) * mod * (gm * q * bce + p)
        return g * torch.where(t > 0, d1, d0), None, None, None


def focal_loss_elem(pred, labels, num_classes, gamma=2.0, alpha=0.25):
    t = F.one_hot(labels, num_classes + 1)[:, :num_classes].type_as(pred)
    return _Focal.apply(pred, t, float(gamma), float(alpha))


def _diou_parts(pred, target, eps):      # iou_loss.py:121-156
    lt = torch.max(pred[:, :2], target[:, :2])
    rb = torch.min(pred[:, 2:], target[:, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    ap = (pred[:, 2] - pred[:, 0]) * (pred[:, 3] - pred[:, 1])
    ag = (target[:, 2] - target[:, 0]) * (target[:, 3] - target[:, 1])
    ious = overlap / (ap + ag - overlap + eps)
    ewh = (torch.max(pred[:, 2:], target[:, 2:]) - torch.min(pred[:, :2], target[:, :2])).clamp(min=0)
    c2 = ewh[:, 0] ** 2 + ewh[:, 1] ** 2 + eps
    left = ((target[:, 0] + target[:, 2]) - (pred[:, 0] + pred[:, 2])) ** 2 / 4
    right = ((target[:, 1] + target[:, 3]) - (pred[:, 1] + pred[:, 3])) ** 2 / 4
    return ious, (left + right) / c2


def box_loss_elem(kind, pred, target, eps=1e-6):
    """The unweighted per-box loss of each kind on decoded xyxy boxes."""
    if kind == 'giou':
        return 1 - O.giou_aligned(pred, target, 1e-6)
    if kind == 'iou':
        return -HR.iou_aligned(pred, target, 1e-6).clamp(min=1e-6).log()
    if kind == 'iou_linear':
        return 1 - HR.iou_aligned(pred, target, 1e-6).clamp(min=1e-6)
    ious, dist = _diou_parts(pred, target, eps)
    if kind == 'diou':
        return 1 - (ious - dist)
    assert kind == 'ciou', kind
    w1, h1 = pred[:, 2] - pred[:, 0], pred[:, 3] - pred[:, 1] + eps
    w2, h2 = target[:, 2] - target[:, 0], target[:, 3] - target[:, 1] + eps
    v = 4 / math.pi ** 2 * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)
    live = v != 0                                                   # DEVIATION: 0 instead of the reference's 0/0 where v == 0
    den = torch.where(live, 1 - ious + v, torch.ones_like(v))
    pen = torch.where(live, v ** 2 / den, torch.zeros_like(v))
    return 1 - (ious - (dist + pen))


def fcos_loss(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, gt_bboxes_ignore=None, opts=None, loss=None, loss_weight=1.0,
              soft_weight=0.0, soft_scale=1.0, num_classes=O.NUM_CLASSES, return_aux=False):
    """head_options_ref.fcos_loss with the loss settings `loss` (loss_settings(...)); box_loss None: by opts['iou_loss']."""
    opts = opts or HR.DEFAULT
    ls = loss_settings(**(loss or {}))
    kind = ls['box_loss'] or ('iou' if opts['iou_loss'] else 'giou')
    B = cls_scores[0].shape[0]
    sizes = [c.shape[-2:] for c in cls_scores]
    pts = O.get_points(sizes)
    labels, tgts, idxs = HR.get_targets(pts, gt_bboxes, gt_labels, opts, num_classes)
    ig_labels = None
    if gt_bboxes_ignore is not None:
        ig_lab = [torch.full((b.shape[0],), num_classes - 1, dtype=torch.long) for b in gt_bboxes_ignore]
        ig_labels, _, _ = HR.get_targets(pts, gt_bboxes_ignore, ig_lab, opts, num_classes)
    dt_ = cls_scores[0].dtype
    stream_w = None
    if loss_weight != 1.0:
        stream_w = []
        for lab in labels:
            w = torch.ones(lab.shape[0], dtype=dt_)
            n = lab.shape[0]
            cut = int(n / 2) if B % 2 == 0 else int(n / B * (B - 1) / 2)
            w[cut:] *= loss_weight
            stream_w.append(w)
        stream_w = torch.cat(stream_w)
    fc = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, num_classes) for c in cls_scores])
    fb = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds])
    fctr = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in centernesses])
    fl, ft = torch.cat(labels), torch.cat(tgts).to(dt_)
    fp = torch.cat([p.repeat(B, 1) for p in pts]).to(dt_)
    pos = ((fl >= 0) & (fl < num_classes)).nonzero().reshape(-1)
    num_pos = max(float(len(pos)), 1.0)
    pb, pc, pt_ = fb[pos], fctr[pos], ft[pos]
    ctr_t = O.centerness_target(pt_)
    denorm = max(float(ctr_t.sum().detach()), 1e-6)
    if len(pos) > 0:
        pp = fp[pos]
        w = torch.ones_like(ctr_t)
        if stream_w is not None:
            w = w * stream_w[pos]
        wb = ctr_t * w
        dp, dt = O.distance2bbox(pp, pb), O.distance2bbox(pp, pt_)
        if not torch.any(wb > 0):                                                     # iou_loss.py:262-266 / :345-348 / :385-388
            loss_bbox = (dp * wb[:, None]).sum()
        else:
            loss_bbox = ls['bbox_weight'] * ((box_loss_elem(kind, dp, dt, ls['box_eps']) * wb).sum() / denorm)
        loss_ctr = ls['ctr_weight'] * ((F.binary_cross_entropy_with_logits(pc, ctr_t, reduction='none') * w).sum() / num_pos)
    else:
        loss_bbox, loss_ctr = pb.sum(), pc.sum()
    weight = torch.ones(fl.shape[0], dtype=dt_)
    if ig_labels is not None:
        fig = torch.cat(ig_labels).clone()
        inter = ((fig - num_classes) * (fl - num_classes)).nonzero().reshape(-1)
        fig[inter] = num_classes
        weight = fig.to(dt_) - num_classes + 1
    if stream_w is not None:
        weight = weight * stream_w
    loss_cls = ls['cls_weight'] * ((focal_loss_elem(fc, fl, num_classes, ls['focal_gamma'], ls['focal_alpha']) * weight[:, None]).sum() / num_pos)
    out = dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_ctr)
    if B % 2 != 0 and soft_weight != 0.0:
        s = 0.0
        for i in range(1, len(cls_scores)):
            h, w_ = cls_scores[i].shape[-2:]
            d = cls_scores[i][B - 2] - cls_scores[i - 1][B - 1][:, :h, :w_]
            s = s + (d * d).mean()
        out['loss_sisoft'] = s * (soft_weight * soft_scale)
    if return_aux:
        return out, dict(labels=fl, bbox_targets=ft, assign_idx=torch.cat(idxs), cls_weight=weight, pos_inds=pos)
    return out


def train_step(sd, img, gt_bboxes, gt_labels, gt_bboxes_ignore=None, opts=None, loss=None, emulate_bf16=False, want_grads=True, **loss_kw):
    """head_options_ref.train_step (ResNet-50 backbone) with the loss settings: returns (losses, gradients by key, aux)."""
    opts = opts or HR.DEFAULT
    q = O.Quant(emulate_bf16)
    tk = HR.trainable_keys(sd)
    p = {k: (v.detach().clone().requires_grad_(k in tk) if v.is_floating_point() else v) for k, v in sd.items()}
    x = q.act(img) if q.on else img
    feats = O.fpn_forward(p, O.resnet50_forward(p, x, q), q)
    cls, reg, ctr = HR.head_forward(p, feats, q, opts, training=True)
    losses, aux = fcos_loss(cls, reg, ctr, gt_bboxes, gt_labels, gt_bboxes_ignore, opts=opts, loss=loss, return_aux=True, **loss_kw)
    total = sum(v for k, v in losses.items() if 'loss' in k)
    grads = {}
    if want_grads:
        total.backward()
        grads = {k: p[k].grad for k in tk}
    aux.update(cls=cls, reg=reg, ctr=ctr)
    return {k: float(v.detach()) for k, v in losses.items()}, grads, aux
