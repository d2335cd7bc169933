"""Fixture of tests/test_aug_test_gpu.py: the REFERENCE's test-time augmentation merge on seeded head outputs.

Container-only (needs the reference tree, through _ref_import.py).  Run:  python tests/golden/make_aug_test.py
Per case it calls the reference's own FCOSHead.get_bboxes(..., rescale=False, with_nms=False) per view, BBoxTestMixin.
merge_aug_bboxes and multiclass_nms (score_factors = centerness), exactly as aug_test_bboxes chains them
(mmdet/models/dense_heads/dense_test_mixins.py:72-104), in both `rescale` modes, and stores inputs and outputs in
aug_test_small.npz (data only).  mmcv's NMS is the greedy stand-in of _ref_import.py, as for every detection fixture here.

Views: A = 96 x 128 and its horizontal mirror, B = 64 x 96 and its vertical mirror; a mirrored view's head outputs are the base
view's, mirrored, plus noise - so candidates of different views overlap and the merged NMS has work to do.  x / y scale factors
differ.  nms_pre = 50: level 0 of both views goes through the top-k.

The generator only accepts a seed for which the comparison is decided by more than fp32 rounding (asserted below):
  * the kept scores are pairwise distinct by > 1e-5 relative;
  * no IoU that decides a kept / suppressed outcome - for every candidate at least as good as the weakest kept box, its largest
    IoU with a better kept box of its class - lies within 1e-3 of the NMS threshold;
  * the top-k boundary of every level that is cut has a gap > 1e-5 relative between the last key in and the first key out.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
from aug_ref import STRIDES, mirror, view_inputs  # noqa: E402  (shared with the tests: one recipe, one mirror)

SUP_CFG = '/root/reference/configs/fcos_semi/r50_caffe_mslonger_tricks_0.Xdata.py'
SIZES_A = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]
SIZES_B = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
VIEWS = [dict(sizes=SIZES_A, img_shape=(96, 128, 3), scale_factor=[1.25, 1.2, 1.25, 1.2], flip=False, flip_direction=None),
         dict(sizes=SIZES_A, img_shape=(96, 128, 3), scale_factor=[1.25, 1.2, 1.25, 1.2], flip=True, flip_direction='horizontal'),
         dict(sizes=SIZES_B, img_shape=(64, 96, 3), scale_factor=[0.9375, 0.8, 0.9375, 0.8], flip=False, flip_direction=None),
         dict(sizes=SIZES_B, img_shape=(64, 96, 3), scale_factor=[0.9375, 0.8, 0.9375, 0.8], flip=True, flip_direction='vertical')]
CFG = dict(nms_pre=50, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)
CASES = [('c80_tricks', 80, False), ('c3_plain', 3, True)]


def make_views(seed, C, exp_decode):
    g = torch.Generator().manual_seed(seed)
    out = []
    for v in VIEWS:
        if not v['flip']:
            base = view_inputs(g, C, v['sizes'], exp_decode)
            out.append(base)
            continue
        cls, raw, ctr = [], [], []
        for c, r, t in zip(*base):
            c, r, t = mirror(c, r, t, v['flip_direction'])
            cls.append(c + 0.3 * torch.randn(c.shape, generator=g))
            raw.append(r + 0.03 * torch.randn(r.shape, generator=g))
            ctr.append(t + 0.3 * torch.randn(t.shape, generator=g))
        out.append((cls, raw, ctr))
    return out


def distances(raw, exp_decode):
    return [torch.exp(r) if exp_decode else torch.relu(r) * s for r, s in zip(raw, STRIDES)]


def iou64(a, b):
    a, b = a.double(), b.double()
    lt, rb = torch.max(a[:, None, :2], b[None, :, :2]), torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
    return inter / (area(a)[:, None] + area(b)[None] - inter)


def run_case(head, views, C, exp_decode):
    core = sys.modules['mmdet.core']
    cfg = R.AttrDict(CFG, nms=R.AttrDict(CFG['nms']))
    metas = [[dict(img_shape=v['img_shape'], scale_factor=np.array(v['scale_factor'], np.float32), flip=v['flip'],
                   flip_direction=v['flip_direction'])] for v in VIEWS]
    aug_b, aug_s, aug_f = [], [], []
    for (cls, raw, ctr), meta in zip(views, metas):
        b, s, f = head.get_bboxes(cls, distances(raw, exp_decode), ctr, meta, cfg, False, False)[0]
        aug_b.append(b)
        aug_s.append(s)
        aug_f.append(f)
        # top-k boundary
        for c, t in zip(cls, ctr):
            P = c.shape[2] * c.shape[3]
            if P > CFG['nms_pre']:
                key = (c.permute(0, 2, 3, 1).reshape(P, C).sigmoid() * t.reshape(P, 1).sigmoid()).max(1)[0].sort(descending=True)[0]
                k = CFG['nms_pre']
                assert (key[k - 1] - key[k]) > 1e-5 * key[k - 1], 'top-k boundary too close'
    mb, ms = head.merge_aug_bboxes(aug_b, aug_s, metas)
    mf = torch.cat(aug_f)
    dets, labels = core.multiclass_nms(mb, ms, cfg.score_thr, cfg.nms, cfg.max_per_img, score_factors=mf)
    assert 20 <= dets.shape[0] <= cfg.max_per_img, dets.shape
    # the decisions are not within rounding
    sc = dets[:, 4].double().sort(descending=True)[0]
    assert ((sc[:-1] - sc[1:]) > 1e-5 * sc[:-1]).all(), 'kept scores too close'
    valid = ms[:, :C] > cfg.score_thr
    final = ms[:, :C] * mf[:, None]
    smin = dets[:, 4].min() if dets.shape[0] == cfg.max_per_img else 0.0
    n_sup = 0
    for c in range(C):
        kb = dets[labels == c]
        if kb.shape[0] == 0:
            continue
        pick = valid[:, c] & (final[:, c] >= smin)
        iou = iou64(mb[pick], kb[:, :4])
        better = kb[None, :, 4] > final[pick, c][:, None]
        worst = torch.where(better, iou, torch.zeros_like(iou)).max(1)[0]      # the IoU that decides the candidate: its largest
        assert ((worst - 0.5).abs() > 1e-3).all(), 'an NMS decision within 1e-3 of the threshold'
        n_sup += int((worst > 0.5).sum())
    assert n_sup >= 20, f'only {n_sup} suppressions: the merge has nothing to do'
    first = dets.new_tensor(VIEWS[0]['scale_factor'])
    not_rescaled = dets.clone()
    not_rescaled[:, :4] *= first                       # dense_test_mixins.py:99-104
    return dets, labels, not_rescaled, int(valid.sum()), n_sup


def main():
    out = dict(strides=np.array(STRIDES), nms_pre=CFG['nms_pre'], score_thr=np.float32(CFG['score_thr']), iou_thr=np.float32(0.5),
               max_per_img=CFG['max_per_img'], sizes_a=np.array(SIZES_A), sizes_b=np.array(SIZES_B))
    for i, v in enumerate(VIEWS):
        out[f'img_shape{i}'] = np.array(v['img_shape'])
        out[f'scale_factor{i}'] = np.array(v['scale_factor'], np.float32)
        out[f'flip{i}'] = np.array(v['flip_direction'] or '')
    for name, C, exp_decode in CASES:
        head = R.build_fcos(SUP_CFG, num_classes=C).bbox_head
        for seed in range(100, 140):
            views = make_views(seed, C, exp_decode)
            try:
                dets, labels, nr, nvalid, nsup = run_case(head, views, C, exp_decode)
            except AssertionError as e:
                print(name, 'seed', seed, 'rejected:', e)
                continue
            break
        else:
            raise SystemExit(f'{name}: no seed accepted')
        print(name, 'seed', seed, 'kept', dets.shape[0], 'valid pairs', nvalid, 'suppressions by kept boxes', nsup)
        out[f'{name}_seed'] = seed
        out[f'{name}_exp_decode'] = int(exp_decode)
        for i, (cls, raw, ctr) in enumerate(views):
            for l in range(5):
                out[f'{name}_v{i}_cls{l}'], out[f'{name}_v{i}_raw{l}'], out[f'{name}_v{i}_ctr{l}'] = \
                    cls[l].numpy(), raw[l].numpy(), ctr[l].numpy()
        out[f'{name}_det_rescale'], out[f'{name}_lab'] = dets.numpy(), labels.numpy()
        out[f'{name}_det_norescale'] = nr.numpy()
    path = os.path.join(HERE, 'aug_test_small.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
