"""torch-CPU restatement of FCOSHead with its options set away from the fcos_semi "tricks" head: forward (anchor_free_head.py:197-217,
fcos_head.py:136-168), targets (:562-705), loss (:170-338) and box decode at test time, for

  center_sampling=False    inside = min(l, t, r, b) > 0                          fcos_head.py:676-678
  norm_on_bbox=False       bbox_pred = exp(scale * x), targets in pixels          fcos_head.py:162-167, :618
  centerness_on_reg=False  conv_centerness reads the classification tower         fcos_head.py:155-158
  loss_bbox=IoULoss        -log(clamp(iou, 1e-6))                                 losses/iou_loss.py:14-36
  conv_bias=False          the tower convolutions have no bias                    mmcv ConvModule bias='auto' with a norm layer

oracle/fcos_oracle.py hard-codes the tricks head; the backbone, the FPN, the bf16 emulation, the points and the loss primitives that
do not depend on the options are imported from it, not copied.  tests/test_head_options_cpu.py pins this file to the reference's own
outputs (tests/golden/*plain*.npz, loss_opt_*.npz) before a GPU test relies on it."""
import torch
import torch.nn.functional as F

from oracle import fcos_oracle as O

DEFAULT = dict(center_sampling=True, norm_on_bbox=True, centerness_on_reg=True, iou_loss=False, conv_bias=True)
PLAIN = dict(center_sampling=False, norm_on_bbox=False, centerness_on_reg=False, iou_loss=True, conv_bias=False)


def options(**kw):
    o = dict(DEFAULT)
    o.update(kw)
    return o


def plain_state_dict(seed=0, num_classes=O.NUM_CLASSES, conv_bias=False, backbone='resnet'):
    """oracle.synth_state_dict (rla_oracle's for backbone='rla') without the tower convolutions' bias keys (conv_bias=False)."""
    if backbone == 'rla':
        from oracle import rla_oracle as RO
        sd = RO.synth_state_dict(seed, num_classes)
    else:
        sd = O.synth_state_dict(seed, num_classes)
    if not conv_bias:
        sd = {k: v for k, v in sd.items() if not is_tower_bias(k)}
    return sd


def is_tower_bias(k):
    return k.startswith(('bbox_head.cls_convs.', 'bbox_head.reg_convs.')) and k.endswith('.conv.bias')


def trainable_keys(sd):
    return O.trainable_keys(sd)


def head_forward(sd, feats, q, opts, training=True):
    cls_scores, bbox_preds, ctrs = [], [], []
    for lvl, x in enumerate(feats):
        cf = rf = x
        for i in range(4):
            cf = F.conv2d(cf, q.wt(sd[f'bbox_head.cls_convs.{i}.conv.weight']), sd.get(f'bbox_head.cls_convs.{i}.conv.bias'), 1, 1)
            cf = q.act(cf, 'tower_pre')
            cf = q.act(F.relu(F.group_norm(cf, 32, sd[f'bbox_head.cls_convs.{i}.gn.weight'], sd[f'bbox_head.cls_convs.{i}.gn.bias'], 1e-5)),
                       'tower_act')
            rf = F.conv2d(rf, q.wt(sd[f'bbox_head.reg_convs.{i}.conv.weight']), sd.get(f'bbox_head.reg_convs.{i}.conv.bias'), 1, 1)
            rf = q.act(rf, 'tower_pre')
            rf = q.act(F.relu(F.group_norm(rf, 32, sd[f'bbox_head.reg_convs.{i}.gn.weight'], sd[f'bbox_head.reg_convs.{i}.gn.bias'], 1e-5)),
                       'tower_act')
        cls = F.conv2d(cf, q.wt(sd['bbox_head.conv_cls.weight']), sd['bbox_head.conv_cls.bias'], 1, 1)
        reg = F.conv2d(rf, q.wt(sd['bbox_head.conv_reg.weight']), sd['bbox_head.conv_reg.bias'], 1, 1)
        src = rf if opts['centerness_on_reg'] else cf                                 # fcos_head.py:155-158
        ctr = F.conv2d(src, q.wt(sd['bbox_head.conv_centerness.weight']), sd['bbox_head.conv_centerness.bias'], 1, 1)
        reg = reg * sd[f'bbox_head.scales.{lvl}.scale']
        if opts['norm_on_bbox']:                                                     # fcos_head.py:162-167
            reg = F.relu(reg)
            if not training:
                reg = reg * O.STRIDES[lvl]
        else:
            reg = reg.exp()
        cls_scores.append(cls)
        bbox_preds.append(reg)
        ctrs.append(ctr)
    return cls_scores, bbox_preds, ctrs


def assign_single(points_per_lvl, gt_bboxes, gt_labels, center_sampling, num_classes=O.NUM_CLASSES):
    """fcos_head.py:623-705.  Returns labels, un-normalised ltrb, argmin index (-1 = background)."""
    if center_sampling:
        return O.assign_single(points_per_lvl, gt_bboxes, gt_labels, num_classes=num_classes)
    pts = torch.cat(points_per_lvl)
    P, G = pts.shape[0], gt_bboxes.shape[0]
    if G == 0:
        return torch.full((P,), num_classes, dtype=torch.long), torch.zeros(P, 4), torch.full((P,), -1, dtype=torch.long)
    lo = torch.cat([torch.full((p.shape[0],), float(r[0])) for p, r in zip(points_per_lvl, O.REGRESS_RANGES)])
    hi = torch.cat([torch.full((p.shape[0],), float(r[1])) for p, r in zip(points_per_lvl, O.REGRESS_RANGES)])
    x, y = pts[:, 0:1], pts[:, 1:2]
    x1, y1, x2, y2 = (gt_bboxes[:, i][None] for i in range(4))
    area = ((x2 - x1) * (y2 - y1)).repeat(P, 1)
    ltrb = torch.stack((x - x1, y - y1, x2 - x, y2 - y), -1)
    inside = ltrb.min(-1)[0] > 0                                                     # fcos_head.py:676-678
    mx = ltrb.max(-1)[0]
    in_range = (mx >= lo[:, None]) & (mx <= hi[:, None])
    area[~inside] = O.INF
    area[~in_range] = O.INF
    min_area, idx = area.min(dim=1)
    labels = gt_labels[idx].clone()
    labels[min_area == O.INF] = num_classes
    tgt = ltrb[torch.arange(P), idx]
    idx = idx.clone()
    idx[min_area == O.INF] = -1
    return labels, tgt, idx


def get_targets(points_per_lvl, gt_bboxes_list, gt_labels_list, opts, num_classes=O.NUM_CLASSES):
    npl = [p.shape[0] for p in points_per_lvl]
    per_img = [assign_single(points_per_lvl, b, l, opts['center_sampling'], num_classes) for b, l in zip(gt_bboxes_list, gt_labels_list)]
    labels, tgts, idxs = [], [], []
    for i in range(len(npl)):
        labels.append(torch.cat([r[0].split(npl)[i] for r in per_img]))
        t = torch.cat([r[1].split(npl)[i] for r in per_img])
        if opts['norm_on_bbox']:
            t = t / O.STRIDES[i]                                                     # fcos_head.py:618-619
        tgts.append(t)
        idxs.append(torch.cat([r[2].split(npl)[i] for r in per_img]))
    return labels, tgts, idxs


def iou_aligned(a, b, eps=1e-6):      # iou2d_calculator.py:212-247 (mode 'iou', is_aligned)
    area1 = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area2 = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = torch.max(area1 + area2 - overlap, a.new_tensor(eps))
    return overlap / union


def fcos_loss(cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, gt_bboxes_ignore=None, opts=None, loss_weight=1.0,
              soft_weight=0.0, soft_scale=1.0, num_classes=O.NUM_CLASSES, return_aux=False):
    """FCOSHead.loss (fcos_head.py:170-338) on the head's outputs (bbox_preds: after relu / exp)."""
    opts = opts or DEFAULT
    B = cls_scores[0].shape[0]
    sizes = [c.shape[-2:] for c in cls_scores]
    pts = O.get_points(sizes)
    labels, tgts, idxs = get_targets(pts, gt_bboxes, gt_labels, opts, num_classes)
    ig_labels = None
    if gt_bboxes_ignore is not None:
        ig_lab = [torch.full((b.shape[0],), num_classes - 1, dtype=torch.long) for b in gt_bboxes_ignore]
        ig_labels, _, _ = get_targets(pts, gt_bboxes_ignore, ig_lab, opts, num_classes)
    stream_w = None
    if loss_weight != 1.0:
        stream_w = []
        for lab in labels:
            w = torch.ones(lab.shape[0])
            n = lab.shape[0]
            cut = int(n / 2) if B % 2 == 0 else int(n / B * (B - 1) / 2)
            w[cut:] *= loss_weight
            stream_w.append(w)
        stream_w = torch.cat(stream_w)
    fc = torch.cat([c.permute(0, 2, 3, 1).reshape(-1, num_classes) for c in cls_scores])
    fb = torch.cat([b.permute(0, 2, 3, 1).reshape(-1, 4) for b in bbox_preds])
    fctr = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in centernesses])
    fl, ft = torch.cat(labels), torch.cat(tgts)
    fp = torch.cat([p.repeat(B, 1) for p in pts])
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
        if not torch.any(wb > 0):                                                     # iou_loss.py:262-266 / :345-348
            loss_bbox = (dp * wb[:, None]).sum()
        elif opts['iou_loss']:
            loss_bbox = (-iou_aligned(dp, dt, 1e-6).clamp(min=1e-6).log() * wb).sum() / denorm      # iou_loss.py:31-35
        else:
            loss_bbox = ((1 - O.giou_aligned(dp, dt, 1e-6)) * wb).sum() / denorm
        loss_ctr = (F.binary_cross_entropy_with_logits(pc, ctr_t, reduction='none') * w).sum() / num_pos
    else:
        loss_bbox, loss_ctr = pb.sum(), pc.sum()
    weight = torch.ones(fl.shape[0])
    if ig_labels is not None:
        fig = torch.cat(ig_labels).clone()
        inter = ((fig - num_classes) * (fl - num_classes)).nonzero().reshape(-1)
        fig[inter] = num_classes
        weight = fig.float() - num_classes + 1
    if stream_w is not None:
        weight = weight * stream_w
    loss_cls = (O.focal_loss_elem(fc, fl, num_classes) * weight[:, None]).sum() / num_pos
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


def train_step(sd, img, gt_bboxes, gt_labels, gt_bboxes_ignore=None, opts=None, emulate_bf16=False, want_grads=True, backbone='resnet',
               **loss_kw):
    """oracle.train_step (backbone='rla': rla_oracle.train_step) with the head options: returns (losses, gradients by key, aux)."""
    opts = opts or DEFAULT
    q = O.Quant(emulate_bf16)
    if backbone == 'rla':
        from oracle import rla_oracle as RO
        tk = RO.trainable_keys(sd)
    else:
        tk = trainable_keys(sd)
    p = {k: (v.detach().clone().requires_grad_(k in tk) if v.is_floating_point() else v) for k, v in sd.items()}
    if backbone == 'rla':
        feats = O.fpn_forward(p, RO.rla_resnet_forward(p, img, q), q)          # (rla_oracle.extract_and_head)
    else:
        x = q.act(img) if q.on else img
        feats = O.fpn_forward(p, O.resnet50_forward(p, x, q), q)
    cls, reg, ctr = head_forward(p, feats, q, opts, training=True)
    losses, aux = fcos_loss(cls, reg, ctr, gt_bboxes, gt_labels, gt_bboxes_ignore, opts=opts, return_aux=True, **loss_kw)
    total = sum(v for k, v in losses.items() if 'loss' in k)
    grads = {}
    if want_grads:
        total.backward()
        grads = {k: p[k].grad for k in tk}
    aux.update(cls=cls, reg=reg, ctr=ctr)
    return {k: float(v) for k, v in losses.items()}, grads, aux
