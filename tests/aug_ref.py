"""fp32 restatement of the reference's test-time augmentation post-processing for the tests (no reference files are read here):
BBoxTestMixin.aug_test_bboxes (mmdet/models/dense_heads/dense_test_mixins.py:38-108) = per view FCOSHead._get_bboxes with
with_nms=False (fcos_head.py:406-548) and bbox_mapping_back (core/bbox/transforms.py:5-55), then multiclass_nms with the
centerness as score factor (core/post_processing/bbox_nms.py:7-94) over mmcv's batched_nms.  tests/test_aug_test_cpu.py pins it
to the reference's own outputs (tests/golden/aug_test_small.npz).  `cap`: the project's deviation - only the best `cap` valid
(location, class) pairs by final score go to the NMS."""
import numpy as np
import torch

STRIDES = (8, 16, 32, 64, 128)
# the test pipeline MultiScaleFlipAug wraps in the tests
NORM = dict(mean=[103.53, 116.28, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False)
TRANSFORMS = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **NORM),
              dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]


def view_inputs(g, C, sizes, exp_decode):
    """Seeded raw head outputs of one view (generator g): cls / ctr logits and the regression conv's raw output x (scale 1) - the
    distance is relu(x) * stride (norm_on_bbox=True) or exp(x) (norm_on_bbox=False).  The fixture's recipe
    (tests/golden/make_aug_test.py) and the GPU tests' own views."""
    cls = [torch.randn(1, C, h, w, generator=g) * 2.0 - 2.0 for h, w in sizes]
    ctr = [torch.randn(1, 1, h, w, generator=g) for h, w in sizes]
    dist = [torch.rand(1, 4, h, w, generator=g) * 5.0 + 0.5 for h, w in sizes]      # in strides
    raw = [torch.log(d * s) for d, s in zip(dist, STRIDES)] if exp_decode else dist
    return cls, raw, ctr


def mirror(cls, raw, ctr, direction):
    """Head outputs [1, C, h, w] of the mirrored image: positions mirrored, the mirrored sides' distances swapped."""
    dims = {'horizontal': [3], 'vertical': [2], 'diagonal': [2, 3]}[direction]
    order = [0, 1, 2, 3]
    if 3 in dims:
        order[0], order[2] = 2, 0
    if 2 in dims:
        order[1], order[3] = 3, 1
    return cls.flip(dims), raw.flip(dims)[:, order], ctr.flip(dims)


def collect(cls, raw, ctr, img_shape, scale_factor, flip_direction, nms_pre, exp_decode):
    """One view: per-level lists of [1, C|4|1, h, w] -> mapped-back boxes [R, 4], scores [R, C], centerness [R]."""
    boxes, scores, cens = [], [], []
    H, W = float(img_shape[0]), float(img_shape[1])
    for c, r, t, s in zip(cls, raw, ctr, STRIDES):
        h, w = c.shape[2:]
        P = h * w
        sc = c[0].permute(1, 2, 0).reshape(P, -1).sigmoid()
        ce = t[0].reshape(P).sigmoid()
        x = r[0].permute(1, 2, 0).reshape(P, 4)
        d = torch.exp(x) if exp_decode else torch.relu(x) * s
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        px, py = (xs.reshape(-1) * s + s // 2).float(), (ys.reshape(-1) * s + s // 2).float()
        if 0 < nms_pre < P:
            # the kernel's documented rule where torch.topk leaves the choice among equal keys open: the first nms_pre of a stable
            # descending sort (ties: the lowest indices, zero keys included), back in index order
            idx = (sc * ce[:, None]).max(1)[0].sort(descending=True, stable=True)[1][:nms_pre].sort()[0]
            sc, ce, d, px, py = sc[idx], ce[idx], d[idx], px[idx], py[idx]
        b = torch.stack([(px - d[:, 0]).clamp(0, W), (py - d[:, 1]).clamp(0, H), (px + d[:, 2]).clamp(0, W), (py + d[:, 3]).clamp(0, H)], 1)
        boxes.append(b)
        scores.append(sc)
        cens.append(ce)
    b = torch.cat(boxes)
    if flip_direction in ('horizontal', 'diagonal'):
        b = torch.stack([W - b[:, 2], b[:, 1], W - b[:, 0], b[:, 3]], 1)
    if flip_direction in ('vertical', 'diagonal'):
        b = torch.stack([b[:, 0], H - b[:, 3], b[:, 2], H - b[:, 1]], 1)
    return b / torch.tensor(np.asarray(scale_factor, np.float32)), torch.cat(scores), torch.cat(cens)


def finish(boxes, scores, cens, score_thr=0.05, iou_thr=0.5, max_per_img=100, cap=None, cap_keeps='lowest'):
    """Returns dets [k, 5], labels [k], and the number of valid pairs.  cap_keeps='highest' is NOT the kernel's rule: the cut through a
    group of equal scores then keeps its highest candidate numbers - for tests that an input can tell the two cuts apart."""
    C = scores.shape[1]
    row, lab = torch.nonzero(scores > score_thr, as_tuple=True)           # (row, class) order
    final = (scores * cens[:, None])[row, lab]
    nvalid = len(row)
    if cap is not None and nvalid > cap:
        if cap_keeps == 'lowest':
            keep = final.sort(descending=True, stable=True)[1][:cap].sort()[0]
        else:
            keep = (nvalid - 1 - final.flip(0).sort(descending=True, stable=True)[1][:cap]).sort()[0]
        row, lab, final = row[keep], lab[keep], final[keep]
    b = boxes[row]
    if len(row) == 0:
        return torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), nvalid
    ob = b + (lab.float() * (b.max() + 1.0))[:, None]
    area = (ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1])
    order = final.sort(descending=True, stable=True)[1]
    sup = torch.zeros(len(row), dtype=torch.bool)
    kept = []
    for i in order.tolist():
        if sup[i]:
            continue
        kept.append(i)
        if len(kept) == max_per_img:
            break
        lt, rb = torch.max(ob[i, :2], ob[:, :2]), torch.min(ob[i, 2:], ob[:, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        sup |= inter / (area[i] + area - inter) > iou_thr
    kept = torch.tensor(kept, dtype=torch.long)
    return torch.cat([b[kept], final[kept, None]], 1), lab[kept], nvalid


def aug_test_bboxes(views, metas, nms_pre, exp_decode, rescale=True, cap=None, cap_keeps='lowest', **nms):
    """views: [(cls, raw, ctr)] per view; metas: dicts with img_shape, scale_factor, flip, flip_direction."""
    parts = [collect(*v, m['img_shape'], m['scale_factor'], m['flip_direction'] if m['flip'] else None, nms_pre, exp_decode)
             for v, m in zip(views, metas)]
    dets, labels, nvalid = finish(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
                                  cap=cap, cap_keeps=cap_keeps, **nms)
    if not rescale:
        dets = dets.clone()
        dets[:, :4] *= torch.tensor(np.asarray(metas[0]['scale_factor'], np.float32))
    return dets, labels, nvalid


def fixture_views(d, name):
    """(views, metas, C, exp_decode) of case `name` of aug_test_small.npz."""
    T = torch.from_numpy
    views = [([T(d[f'{name}_v{i}_cls{l}']) for l in range(5)], [T(d[f'{name}_v{i}_raw{l}']) for l in range(5)],
              [T(d[f'{name}_v{i}_ctr{l}']) for l in range(5)]) for i in range(4)]
    metas = [dict(img_shape=tuple(int(x) for x in d[f'img_shape{i}']), scale_factor=d[f'scale_factor{i}'],
                  flip=bool(str(d[f'flip{i}'])), flip_direction=str(d[f'flip{i}']) or None) for i in range(4)]
    return views, metas, views[0][0][0].shape[1], bool(int(d[f'{name}_exp_decode']))


def match(got_b, got_l, ref_b, ref_l):
    """The single-view parity test's criteria (tests/test_sweep_gpu.py::_match): same count, same scores in the same order, the
    same labels and boxes once both sides are ordered by (score, label, x1)."""
    got_b, got_l, ref_b, ref_l = (torch.as_tensor(x).cpu() for x in (got_b, got_l, ref_b, ref_l))
    assert got_b.shape[0] == ref_b.shape[0], (got_b.shape, ref_b.shape)
    assert torch.allclose(got_b[:, 4], ref_b[:, 4], rtol=1e-4, atol=1e-6)
    o_ref = np.lexsort((ref_b[:, 0].numpy(), ref_l.numpy(), -ref_b[:, 4].numpy()))
    o_got = np.lexsort((got_b[:, 0].numpy(), got_l.numpy(), -got_b[:, 4].numpy()))
    assert torch.equal(got_l[o_got], ref_l[o_ref])
    assert torch.allclose(got_b[o_got], ref_b[o_ref], rtol=1e-4, atol=1e-3)
