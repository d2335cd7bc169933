"""Generate the ATSS fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_atss_golden.py
  atss_<case>.npz   the reference's ATSSHead (configs/atss/atss_r50_fpn_1x_coco.py's bbox_head / train_cfg) on a 128 x 160 canvas at
                    batch 2: its AnchorGenerator, valid flags, ATSSAssigner.assign, DeltaXYWHBBoxCoder (bbox2delta / delta2bbox),
                    bbox_overlaps, ATSSHead.centerness_target and ATSSHead.loss with autograd - inputs and outputs only.
Cases: a  1-40 random boxes;  b  an image with no box;  c  heavily overlapping boxes that share candidates;  d  a box whose centre
lies within 4 px of the border;  e  the second image with pad_shape (96, 128);  f  topk = 3, anchor_scale = 4.
Before a case is written it is checked, and redrawn (next seed) if it violates one of: (1) for every (box, level) the k-th and
(k+1)-th distances differ in fp32; (2) no candidate IoU lies within 1e-5 (relative) of its threshold, computed in float64; (3) no
anchor is positive for two boxes at equal IoU; (4) no centerness target is NaN.
Layout (level-major [level][image][y][x], as the kernels' buffers): labels, assign_idx (-1 = none), cls_weight, targets (the
assigned ground-truth box), deltas (the reference's encoded bbox_targets), npos, num_total = sum_i max(npos_i, 1); the head outputs
cls{l} / reg{l} (the box predictor's output in front of Scale) / ctr{l}, scales; the three losses, their gradients, the decoded
boxes and centerness targets of the positives, the sum of the centerness targets."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, save  # noqa: E402

CFG = '/root/reference/configs/atss/atss_r50_fpn_1x_coco.py'
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
STRIDES = (8, 16, 32, 64, 128)
H, W = 128, 160


def install():
    R.install()
    for n in ('mmdet.core.bbox.assigners', 'mmdet.core.bbox.samplers', 'mmdet.core.bbox.coder', 'mmdet.core.anchor'):
        if n not in sys.modules:
            m = types.ModuleType(n)
            m.__path__ = [R.REF + '/' + n.replace('.', '/')]
            sys.modules[n] = m
    imp = importlib.import_module
    core = sys.modules['mmdet.core']
    sys.modules['mmdet.utils'].util_mixins = imp('mmdet.utils.util_mixins')
    bb = imp('mmdet.core.bbox.builder')
    ib = imp('mmdet.core.bbox.iou_calculators.builder')
    sys.modules['mmdet.core.bbox.iou_calculators'].build_iou_calculator = ib.build_iou_calculator
    for leaf in ('assigners.atss_assigner', 'samplers.pseudo_sampler', 'coder.delta_xywh_bbox_coder'):
        imp('mmdet.core.bbox.' + leaf)
    ab = imp('mmdet.core.anchor.builder')
    imp('mmdet.core.anchor.anchor_generator')
    au = imp('mmdet.core.anchor.utils')
    misc = imp('mmdet.core.utils.misc')
    core.anchor_inside_flags, core.images_to_levels = au.anchor_inside_flags, au.images_to_levels
    core.unmap = misc.unmap
    core.build_anchor_generator = ab.build_anchor_generator
    core.build_assigner, core.build_sampler, core.build_bbox_coder = bb.build_assigner, bb.build_sampler, bb.build_bbox_coder
    imp('mmdet.models.dense_heads.anchor_head')
    return imp('mmdet.models.dense_heads.atss_head')


def build_head(num_classes, topk, anchor_scale):
    mod = install()
    cfg = R.load_cfg(CFG)['model']
    hc = dict(cfg['bbox_head'], num_classes=num_classes)
    hc.pop('type')
    hc['anchor_generator'] = dict(hc['anchor_generator'], octave_base_scale=anchor_scale)
    tc = R.AttrDict(cfg['train_cfg'])
    tc['assigner'] = dict(tc['assigner'], topk=topk)
    head = mod.ATSSHead(train_cfg=tc, test_cfg=R.AttrDict(cfg['test_cfg']), **hc)
    head.train()
    return head


def boxes_for(case, rng, img):
    def rand(n, lo=6.0, hi=110.0):
        w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        x, y = rng.uniform(0, W - 4, n), rng.uniform(0, H - 4, n)
        return np.stack([x, y, np.minimum(x + w, W - 0.5), np.minimum(y + h, H - 0.5)], 1).astype(np.float32)
    if case == 'b' and img == 1:
        return np.zeros((0, 4), np.float32)
    if case == 'c':          # one cluster: near-identical centres, sizes within 25 % of each other
        n = 6
        cx, cy, s = rng.uniform(60, 100), rng.uniform(50, 80), rng.uniform(40, 60)
        c = np.stack([cx + rng.uniform(-5, 5, n), cy + rng.uniform(-5, 5, n)], 1)
        wh = s * rng.uniform(0.8, 1.25, (n, 2))
        return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    if case == 'd':          # the first box: centre within 4 px of the left / top border
        b = rand(4)
        if img == 0:
            b[0] = (0.0, rng.uniform(20.0, 40.0), rng.uniform(4.0, 7.5), rng.uniform(70.0, 100.0))
        else:
            b[0] = (rng.uniform(30.0, 50.0), 0.0, rng.uniform(100.0, 130.0), rng.uniform(4.0, 7.5))
        return b
    return rand(int(rng.randint(1, 41)) if case == 'a' else int(rng.randint(2, 9)))


def reference_assignment(head, gts, gls, metas):
    """The reference's own anchors, valid flags and ATSSAssigner.assign per image -> assigned ground-truth index per anchor (-1 =
    none / invalid), max IoU, in the image's level order; and everything the generator's checks need."""
    anchor_list, valid_list = head.get_anchors(SIZES, metas, device='cpu')
    out = []
    for i, (gt, gl) in enumerate(zip(gts, gls)):
        flat, valid = torch.cat(anchor_list[i]), torch.cat(valid_list[i])
        nl = [int(v.sum()) for v in valid_list[i]]
        idx = torch.full((flat.shape[0],), -1, dtype=torch.long)
        if len(gt):
            res = head.assigner.assign(flat[valid], nl, gt, None, gl)
            idx[valid] = res.gt_inds - 1
        out.append((flat, valid, nl, idx))
    return out


def check_case(head, gts, ref, topk):
    """The four conditions of the module docstring; returns a reason string, or None when the case is clean."""
    from mmdet.core.bbox.iou_calculators.iou2d_calculator import bbox_overlaps
    for (flat, valid, nl, idx), gt in zip(ref, gts):
        if not len(gt):
            continue
        a = flat[valid]
        acx, acy = (a[:, 0] + a[:, 2]) / 2.0, (a[:, 1] + a[:, 3]) / 2.0
        gcx, gcy = (gt[:, 0] + gt[:, 2]) / 2.0, (gt[:, 1] + gt[:, 3]) / 2.0
        dist = ((acx[:, None] - gcx[None]).pow(2) + (acy[:, None] - gcy[None]).pow(2)).sqrt()
        iou64 = bbox_overlaps(a.double(), gt.double())
        iou32 = bbox_overlaps(a, gt)
        pos = torch.zeros_like(iou32, dtype=torch.bool)
        for g in range(len(gt)):
            cand, s = [], 0
            for n in nl:
                d = dist[s:s + n, g]
                k = min(topk, n)
                srt = d.sort()[0]
                if k < n and srt[k - 1] == srt[k]:
                    return f'distance tie at the cut (box {g})'
                cand.append(d.topk(k, largest=False)[1] + s)
                s += n
            cand = torch.cat(cand)
            v = iou64[cand, g]
            thr = v.mean() + v.std()
            if bool(((v - thr).abs() <= 1e-5 * thr.abs()).any()):
                return f'candidate IoU at its threshold (box {g})'
            cx, cy = acx[cand].double(), acy[cand].double()
            inside = torch.stack([cx - gt[g, 0], cy - gt[g, 1], gt[g, 2] - cx, gt[g, 3] - cy], 1).min(1)[0] > 0.01
            pos[cand[(v >= thr) & inside], g] = True
        for m in (pos.sum(1) > 1).nonzero().view(-1):
            v = iou32[m][pos[m]]
            if len(torch.unique(v)) < len(v):
                return 'an anchor positive for two boxes at equal IoU'
        # the reference's assignment is the one these candidates give
        want = torch.where(pos.any(1), torch.where(pos, iou32, torch.full_like(iou32, -1.0)).argmax(1), torch.full((len(a),), -1, dtype=torch.long))
        assert torch.equal(want, idx[valid]), 'the generator\'s reading of the candidates differs from ATSSAssigner.assign'
    return None


def gen_case(case, seed):
    topk, scale, C = (3, 4, 18) if case == 'f' else (9, 8, 80 if case == 'a' else 20)      # (20 classes: smaller files)
    head = build_head(C, topk, scale)
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    gts = [torch.from_numpy(boxes_for(case, rng, i)) for i in range(2)]
    gls = [torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')) for b in gts]
    pads = [(H, W), (96, 128) if case == 'e' else (H, W)]
    metas = [dict(img_shape=(p[0], p[1], 3), pad_shape=(p[0], p[1], 3)) for p in pads]
    ref = reference_assignment(head, gts, gls, metas)
    why = check_case(head, gts, ref, topk)
    if why:
        return why
    # head outputs: logits around the focal prior, deltas of a few tenths .. a few units, some beyond the dw / dh clamp
    cls = [(torch.randn(2, C, h, w, generator=g) * 1.5 - 2.5).requires_grad_() for h, w in SIZES]
    reg = [torch.randn(2, 4, h, w, generator=g) * 3.0 for h, w in SIZES]
    reg[0][0, 2, ::3, ::4] = 30.0           # scale * 30 * 0.2 > |log(16 / 1000)|: an active clamp (some of them on positives, asserted)
    reg[1][:, 3, ::2, ::3] = -28.0
    reg = [r.requires_grad_() for r in reg]
    ctr = [torch.randn(2, 1, h, w, generator=g).requires_grad_() for h, w in SIZES]
    scales = (torch.rand(5, generator=g) * 0.6 + 0.7).requires_grad_()
    pred = [r * scales[i] for i, r in enumerate(reg)]
    losses = head.loss(cls, pred, ctr, gts, gls, metas)
    total = sum(sum(v) for v in losses.values())
    total.backward()
    # targets in the kernels' layout
    anchor_list, valid_list = head.get_anchors(SIZES, metas, device='cpu')
    tg = head.get_targets(anchor_list, valid_list, gts, metas, gt_labels_list=gls, label_channels=C)
    _, labels_l, lw_l, bt_l, _, num_total, _ = tg
    labels = torch.cat([x.reshape(-1) for x in labels_l])
    weight = torch.cat([x.reshape(-1) for x in lw_l])
    deltas = torch.cat([x.reshape(-1, 4) for x in bt_l])
    split = [h * w for h, w in SIZES]
    per = [r[3].split(split) for r in ref]
    aidx = torch.cat([per[i][l] for l in range(5) for i in range(2)])
    targets = torch.zeros(len(labels), 4)
    fresh = head.get_anchors(SIZES, metas, device='cpu')[0]          # (get_targets concatenated anchor_list in place)
    anchors_lm = torch.cat([torch.cat([fresh[i][l] for i in range(2)]) for l in range(5)])
    img_of = torch.cat([torch.cat([torch.full((split[l],), i) for i in range(2)]) for l in range(5)])
    pos = (labels < C).nonzero().view(-1)
    assert torch.equal(pos, (aidx >= 0).nonzero().view(-1))
    for m in pos.tolist():
        i = int(img_of[m])
        targets[m] = gts[i][aidx[m]]
        assert int(labels[m]) == int(gls[i][aidx[m]])
    npos = [int(((img_of == i) & (labels < C)).sum()) for i in range(2)]
    assert num_total == sum(max(n, 1) for n in npos)
    d = dict(sizes=np.array(SIZES), B=2, num_classes=C, topk=topk, anchor_scale=float(scale), stds=np.array(head.bbox_coder.stds, np.float32),
             bbox_weight=float(head.loss_bbox.loss_weight), pads=np.array(pads), labels=labels, assign_idx=aidx.int(), cls_weight=weight,
             targets=targets, deltas=deltas, npos=np.array(npos), num_total=int(num_total), scales=scales.detach(), gscales=scales.grad)
    if len(pos):
        flat_pred = torch.cat([p.permute(0, 2, 3, 1).reshape(-1, 4) for p in pred]).detach()
        ct = head.centerness_target(anchors_lm[pos], deltas[pos])
        assert not bool(torch.isnan(ct).any())
        dec = head.bbox_coder.decode(anchors_lm[pos], flat_pred[pos])
        d.update(pos=pos, ctr_targets=ct, ctr_sum=float(ct.sum()), decoded=dec, anchors_pos=anchors_lm[pos])
        if case != 'b':
            dwh = flat_pred[pos][:, 2:] * torch.tensor(head.bbox_coder.stds[2:])
            assert bool((dwh.abs() > abs(np.log(16 / 1000))).any()), 'no positive with an active dw / dh clamp: change the seed'
    else:
        d.update(pos=np.zeros(0, np.int64), ctr_sum=0.0)
    for i in range(2):
        d[f'gt{i}'], d[f'gl{i}'] = gts[i], gls[i]
    for l in range(5):
        d[f'cls{l}'], d[f'reg{l}'], d[f'ctr{l}'] = cls[l].detach(), reg[l].detach(), ctr[l].detach()
        d[f'gcls{l}'], d[f'greg{l}'], d[f'gctr{l}'] = cls[l].grad, reg[l].grad, ctr[l].grad
    for k, v in losses.items():
        d[k] = np.float64(float(sum(v)))
        assert np.isfinite(d[k]), k
    print(case, 'seed', seed, 'npos', npos, {k: float(d[k]) for k in losses})
    save(f'atss_{case}.npz', **d)
    return None


if __name__ == '__main__':
    torch.set_num_threads(8)
    for ci, case in enumerate('abcdef'):
        for t in range(50):
            try:
                why = gen_case(case, 1000 * (ci + 1) + t)
            except AssertionError as e:
                why = str(e)
            if why is None:
                break
            print(case, 'redraw:', why)
        else:
            raise SystemExit(f'case {case}: no clean draw')
