"""Generate the FoveaBox fixtures by running the REFERENCE's own python on CPU.

Container-only (needs /root/reference).  Run:  python tests/golden/make_fovea_golden.py
  fovea_<case>.npz   the reference's FoveaHead (configs/foveabox/fovea_r50_fpn_4x4_1x_coco.py's bbox_head with GN-32 towers) on a
                     128 x 160 canvas at batch 2: its get_targets, its loss with autograd and its get_bboxes (with the stand-in
                     NMS of _ref_import.py, as make_detect_many.py uses it) - inputs and outputs only.
Cases: a  80 classes, 1-40 random boxes, the config's scale_ranges;  b  the second image without boxes;  c  scale_ranges that no box
hits (num_pos 0);  d  nested boxes on one level, a box that hits two levels, a box whose fovea is empty at its level and a box whose
fovea lies wholly beyond the right / bottom edge of its level;  e  18 classes, sigma 0.25, base_edge_list (8 .. 128), scale_ranges
((1, 16) .. (64, 512)) with positives on all five levels, beta 1, gamma 2, alpha 0.25, loss weights 2 / 0.5.
A case is redrawn (next seed) unless, computed in float64: no two hits of a level in an image have equal fp32 sqrt-areas; no
sqrt-area lies within 1e-5 (relative) of a bound; no ceil / floor argument lies within 1e-4 of an integer; no raw target lies within
1e-6 (relative) of 1/16 or 16; no positive has |pred - target| within 1e-6 of beta.
Layout (level-major [level][image][y][x], as the kernels' buffers): labels, assign_idx (the winning box's index in its image, -1 =
none: the reference's own painting, run once more with the box indices as labels), pos (the positives' locations), log_targets (at
`pos` only: the reference leaves uninitialised memory elsewhere), num_pos; the head outputs cls{l} / reg{l}; the two losses and their
gradients gcls{l} / greg{l}; det{i}_boxes (with scores) / det{i}_labels of get_bboxes(rescale=True); head_keys (case a): the
reference head's state_dict keys."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R, save  # noqa: E402

CFG = '/root/reference/configs/foveabox/fovea_r50_fpn_4x4_1x_coco.py'
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
STRIDES = (8, 16, 32, 64, 128)
H, W = 128, 160
TEST_CFG = dict(nms_pre=100, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
IMG_SHAPES = [(H, W, 3), (100, 130, 3)]          # the second image: the clamp to img_shape - 1 bites
SCALE_FACTORS = [np.ones(4, np.float32), np.full(4, 1.25, np.float32)]


def install():
    R.install()
    ops = sys.modules['mmcv.ops']
    if not hasattr(ops, 'DeformConv2d'):          # fovea_head.py imports it for FeatureAlign (with_deform=True), never built here
        ops.DeformConv2d = type('DeformConv2d', (nn.Module,), {})
    cnn = sys.modules['mmcv.cnn']
    if not hasattr(cnn, 'normal_init'):
        cnn.normal_init = None
    importlib.import_module('mmdet.models.losses.smooth_l1_loss')
    return importlib.import_module('mmdet.models.dense_heads.fovea_head')


def build_head(num_classes, **over):
    mod = install()
    hc = dict(R.load_cfg(CFG)['model']['bbox_head'], num_classes=num_classes, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
    hc.pop('type')
    hc.update(over)
    tc = R.AttrDict(TEST_CFG, nms=R.AttrDict(TEST_CFG['nms']))
    head = mod.FoveaHead(train_cfg=R.AttrDict(), test_cfg=tc, **hc)
    head.train()
    return head


def boxes_for(case, rng, img):
    def rand(n, lo=6.0, hi=110.0, log=False):
        if log:
            w, h = np.exp(rng.uniform(np.log(lo), np.log(hi), n)), np.exp(rng.uniform(np.log(lo), np.log(hi), n))
        else:
            w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        x, y = rng.uniform(0, W - 4, n), rng.uniform(0, H - 4, n)
        return np.stack([x, y, np.minimum(x + w, W - 0.5), np.minimum(y + h, H - 0.5)], 1).astype(np.float32)
    if case == 'b' and img == 1:
        return np.zeros((0, 4), np.float32)
    if case == 'd' and img == 0:
        j = rng.uniform(-0.2, 0.2, (5, 4))
        b = np.array([[20, 20, 80, 80],           # sqrt-area 60: hits levels 0 (1, 64) and 1 (32, 128)
                      [40, 40, 60, 60],           # nested in it on level 0: painted later, wins its cells
                      [30, 26, 70, 74],           # nested too, between the two in area
                      [13, 13, 18, 18],           # its fovea lies between two cell centres of level 0: paints nothing
                      [170, 140, 200, 170]],      # its fovea lies beyond the right and the bottom edge: paints the corner cell
                     np.float64) + j
        return b.astype(np.float32)
    if case == 'e':
        return rand(int(rng.randint(10, 25)), 3.0, 150.0, log=True)
    return rand(int(rng.randint(1, 41)) if case == 'a' else int(rng.randint(2, 9)))


def check_case(head, gts, flat_pred, labels, targets_raw, log_targets, pos, beta):
    """The clean-draw conditions of the module docstring; returns a reason string, or None when the case is clean."""
    sigma = head.sigma
    for gt in gts:
        if not len(gt):
            continue
        a32 = torch.sqrt((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))
        a64 = torch.sqrt((gt[:, 2].double() - gt[:, 0].double()) * (gt[:, 3].double() - gt[:, 1].double()))
        for (lo, hi), s in zip(head.scale_ranges, STRIDES):
            for bnd in (lo, hi):
                if bool(((a64 - bnd).abs() <= 1e-5 * bnd).any()):
                    return 'a sqrt-area at a bound'
            hit = (a32 >= lo) & (a32 <= hi)
            if len(torch.unique(a32[hit])) < int(hit.sum()):
                return 'two hits of a level with equal fp32 sqrt-area'
            b = gt[hit].double() / s
            for o in (0, 1):
                half = 0.5 * (b[:, 2 + o] - b[:, o])
                for arg in (b[:, o] + (1 - sigma) * half - 0.5, b[:, o] + (1 + sigma) * half - 0.5):
                    if bool(((arg - arg.round()).abs() <= 1e-4).any()):
                        return 'a ceil / floor argument at an integer'
    if len(pos):
        r = targets_raw.double()
        for bnd in (1.0 / 16.0, 16.0):
            if bool(((r - bnd).abs() <= 1e-6 * bnd).any()):
                return 'a raw target at a clamp bound'
        d = (flat_pred[pos].double() - log_targets.double()).abs()
        if bool(((d - beta).abs() <= 1e-6).any()):
            return '|pred - target| at beta'
    return None


def raw_targets(head, gts, aidx, img_of, lvl_of, pts, pos):
    """The positives' unclamped targets from their winning boxes, float64 (for the clean-draw conditions only)."""
    out = torch.zeros(len(pos), 4, dtype=torch.float64)
    for k, m in enumerate(pos.tolist()):
        g = gts[int(img_of[m])][int(aidx[m])].double()
        bl = float(head.base_edge_list[int(lvl_of[m])])
        px, py = float(pts[m, 0]), float(pts[m, 1])
        out[k] = torch.tensor([(px - g[0]) / bl, (py - g[1]) / bl, (g[2] - px) / bl, (g[3] - py) / bl])
    return out


def gen_case(case, seed):
    C = 80 if case == 'a' else 18 if case == 'e' else 20
    over = {}
    if case == 'c':
        over = dict(scale_ranges=((1000, 2000),) * 5)
    if case == 'e':
        over = dict(sigma=0.25, base_edge_list=(8, 16, 32, 64, 128), scale_ranges=((1, 16), (8, 32), (16, 64), (32, 128), (64, 512)),
                    loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
                    loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=0.5))
    head = build_head(C, **over)
    beta = float(head.loss_bbox.beta)
    rng = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    gts = [torch.from_numpy(boxes_for(case, rng, i)) for i in range(2)]
    gls = [torch.from_numpy(rng.randint(0, C, len(b)).astype('int64')) for b in gts]
    # head outputs: logits around the focal prior, box predictions N(0, 1.5) (both SmoothL1 branches occur on positives)
    cls = [(torch.randn(2, C, h, w, generator=g) * 1.5 - 2.5).requires_grad_() for h, w in SIZES]
    reg = [(torch.randn(2, 4, h, w, generator=g) * 1.5).requires_grad_() for h, w in SIZES]
    points = head.get_points(SIZES, torch.float32, 'cpu')
    labels, log_t = head.get_targets(gts, gls, SIZES, points)
    # the winning box of every painted cell: the reference's painting with the box indices as labels
    nc = head.num_classes
    head.num_classes = 1 << 20
    aidx, _ = head.get_targets(gts, [torch.arange(len(b)) for b in gts], SIZES, points)
    head.num_classes = nc
    aidx = torch.where(aidx == (1 << 20), torch.full_like(aidx, -1), aidx)
    pos = (labels < C).nonzero().view(-1)
    assert torch.equal(pos, (aidx >= 0).nonzero().view(-1))
    split = [h * w for h, w in SIZES]
    img_of = torch.cat([torch.cat([torch.full((split[l],), i) for i in range(2)]) for l in range(5)])
    lvl_of = torch.cat([torch.full((2 * split[l],), l) for l in range(5)])
    pts = torch.cat([torch.stack([STRIDES[l] * points[l][1].reshape(-1), STRIDES[l] * points[l][0].reshape(-1)], 1).repeat(2, 1) for l in range(5)])
    for m in pos.tolist():
        assert int(labels[m]) == int(gls[int(img_of[m])][int(aidx[m])])
    flat_pred = torch.cat([p.permute(0, 2, 3, 1).reshape(-1, 4) for p in reg]).detach()
    why = check_case(head, gts, flat_pred, labels, raw_targets(head, gts, aidx, img_of, lvl_of, pts, pos), log_t[pos], pos, beta)
    if why:
        return why
    npos_img = [int(((img_of == i) & (labels < C)).sum()) for i in range(2)]
    if case == 'b':
        assert npos_img[1] == 0 and npos_img[0] > 0
    if case == 'c':
        assert len(pos) == 0
    if case == 'e':
        assert all(int(((lvl_of == l) & (labels < C)).sum()) > 0 for l in range(5)), 'a level without positives: change the seed'
    if case == 'd':
        i0 = aidx[:320].reshape(16, 20)                                   # level 0, image 0
        l1 = aidx[2 * 320:2 * 320 + 80]                                   # level 1, image 0
        assert bool((i0 == 1).any()) and bool((i0 == 2).any()) and bool((i0 == 0).any()), 'nested boxes: all three must own cells'
        assert bool((l1 == 0).any()), 'box 0 must also paint level 1'
        assert not bool((i0 == 3).any()), 'box 3 must paint nothing'
        assert int(i0[15, 19]) == 4 and int((i0 == 4).sum()) == 1, 'box 4 must paint the corner cell only'
    if len(pos):
        d = (flat_pred[pos] - log_t[pos]).abs()
        assert bool((d < beta).any()) and bool((d >= beta).any()), 'both SmoothL1 branches must occur on positives: change the seed'
    metas = [dict(img_shape=s, scale_factor=f) for s, f in zip(IMG_SHAPES, SCALE_FACTORS)]
    losses = head.loss(cls, reg, gts, gls, metas)
    (losses['loss_cls'] + losses['loss_bbox']).backward() if len(pos) else losses['loss_cls'].backward()
    with torch.no_grad():
        dets = head.get_bboxes([c.detach() for c in cls], [r.detach() for r in reg], metas, rescale=True)
    d = dict(sizes=np.array(SIZES), B=2, num_classes=C, sigma=float(head.sigma), base_edge_list=np.array(head.base_edge_list, np.float32),
             scale_ranges=np.array(head.scale_ranges, np.float32), beta=beta, gamma=float(head.loss_cls.gamma), alpha=float(head.loss_cls.alpha),
             cls_weight=float(head.loss_cls.loss_weight), bbox_weight=float(head.loss_bbox.loss_weight),
             labels=labels, assign_idx=aidx.int(), pos=pos, log_targets=log_t[pos], num_pos=len(pos), npos_img=np.array(npos_img),
             img_shapes=np.array([s[:2] for s in IMG_SHAPES]), scale_factors=np.stack(SCALE_FACTORS),
             nms_pre=TEST_CFG['nms_pre'], score_thr=TEST_CFG['score_thr'], iou_thr=TEST_CFG['nms']['iou_threshold'],
             max_per_img=TEST_CFG['max_per_img'])
    for i in range(2):
        d[f'gt{i}'], d[f'gl{i}'] = gts[i], gls[i]
        d[f'det{i}_boxes'], d[f'det{i}_labels'] = dets[i][0], dets[i][1]
    for l in range(5):
        d[f'cls{l}'], d[f'reg{l}'] = cls[l].detach(), reg[l].detach()
        d[f'gcls{l}'] = cls[l].grad
        d[f'greg{l}'] = reg[l].grad if reg[l].grad is not None else torch.zeros_like(reg[l])
    for k, v in losses.items():
        d[k] = np.float64(float(v))
        assert np.isfinite(d[k]), k
    if case == 'a':
        d['head_keys'] = np.array(['bbox_head.' + k for k in head.state_dict().keys()])
    print(case, 'seed', seed, 'npos', npos_img, {k: float(d[k]) for k in losses}, 'dets', [len(x[1]) for x in dets])
    save(f'fovea_{case}.npz', **d)
    return None


if __name__ == '__main__':
    torch.set_num_threads(8)
    for ci, case in enumerate('abcde'):
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
