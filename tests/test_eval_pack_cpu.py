"""pack_eval_inputs / flatten_annotations (the host side of the on-device evaluator) on CPU tensors: a hand-written case of
3 images x 3 categories - cell order and offsets, the rank cut, the score permutation under ties, the dropped foreign
category and `area` overriding w * h."""
import numpy as np
import torch

from dsl_amd import evaluation as E

IMG_IDS, CAT_IDS = [10, 20, 30], [1, 2, 5]


def _triple():
    # (label, score) per slot; K = 5 slots, `count` valid per image.  Boxes carry the flat row index so that rows are traceable.
    rows = [[(0, .5), (0, .9), (0, .5), (2, .7), (1, .99)],       # image 0: 4 valid (slot 4 is past count)
            [(0, .5), (1, .25), (0, .9), (0, 0), (0, 0)],          # image 1: 3 valid
            [(1, .25), (0, 0), (0, 0), (0, 0), (0, 0)]]            # image 2: 1 valid
    dets, labels = torch.zeros(3, 5, 5), torch.zeros(3, 5, dtype=torch.int64)
    for i, r in enumerate(rows):
        for k, (lab, s) in enumerate(r):
            n = i * 5 + k
            dets[i, k] = torch.tensor([n, n, n + 10., n + 20., s])
            labels[i, k] = lab
    return dets, labels, torch.tensor([4, 3, 1], dtype=torch.int32)


def _anns():
    return [[dict(bbox=[0., 0., 10., 10.], category_id=1, iscrowd=0), dict(bbox=[1., 1., 2., 2.], category_id=99, iscrowd=0),
             dict(bbox=[5., 5., 4., 4.], category_id=1, iscrowd=1, area=33.0)],
            [dict(bbox=[2., 3., 4., 5.], category_id=5)],
            [dict(bbox=[7., 7., 3., 3.], category_id=2, iscrowd=0), dict(bbox=[6., 6., 2., 8.], category_id=1, iscrowd=0)]]


def test_cells_offsets_rank_cut_and_permutation():
    dets, labels, count = _triple()
    p = E.pack_eval_inputs(dets, labels, count, _anns(), IMG_IDS, CAT_IDS, 'coco', max_dets=2)
    # (category, image, rank): category 0 has .9 (row 1), .5 (row 0) of image 0 - the second .5 (row 2) is rank 2 and cut - then
    # .9 (row 7), .5 (row 5) of image 1; category 1: row 6 (image 1), row 10 (image 2); category 2: row 3
    assert p.det_src.tolist() == [1, 0, 7, 5, 6, 10, 3]
    assert p.det_off.dtype == torch.int32 and p.det_off.tolist() == [0, 2, 4, 4, 4, 5, 6, 7, 7, 7]
    assert p.det_boxes.dtype == torch.float32 and p.det_boxes[:, 0].tolist() == [1., 0., 7., 5., 6., 10., 3.]
    assert torch.equal(p.det_scores, torch.tensor([.9, .5, .9, .5, .25, .25, .7]))
    # per category by descending score; the equal .9s and .5s of category 0 by image, the equal .25s of category 1 by image
    assert p.perm.dtype == torch.int32 and p.perm.tolist() == [0, 2, 1, 3, 4, 5, 6]
    assert (p.num_cats, p.num_imgs) == (3, 3)


def test_no_cut_keeps_array_order_among_equal_scores():
    dets, labels, count = _triple()
    p = E.pack_eval_inputs(dets, labels, count, _anns(), IMG_IDS, CAT_IDS, 'coco', max_dets=None)
    assert p.det_src.tolist() == [1, 0, 2, 7, 5, 6, 10, 3]           # rows 0 and 2 (.5, .5) stay in array order
    assert p.det_off.tolist() == [0, 3, 5, 5, 5, 6, 7, 8, 8, 8]
    assert p.perm.tolist() == [0, 3, 1, 2, 4, 5, 6, 7]
    p1 = E.pack_eval_inputs(dets, labels, count, _anns(), IMG_IDS, CAT_IDS, 'coco', max_dets=1)
    assert p1.det_src.tolist() == [1, 7, 6, 10, 3] and p1.perm.tolist() == [0, 1, 2, 3, 4]


def test_ground_truth_flattening():
    gt = E.flatten_annotations(_anns(), IMG_IDS, CAT_IDS, 'coco')
    # category 1: image 0's two boxes in annotation order, image 2's; category 2: image 2's; category 5: image 1's.  99 is dropped.
    assert gt.boxes.tolist() == [[0., 0., 10., 10.], [5., 5., 4., 4.], [6., 6., 2., 8.], [7., 7., 3., 3.], [2., 3., 4., 5.]]
    assert gt.area.tolist() == [100., 33., 16., 9., 20.]               # `area` overrides w * h
    assert gt.crowd.tolist() == [0, 1, 0, 0, 0] and gt.ignore.tolist() == [0] * 5
    assert gt.off.dtype == np.int32 and gt.off.tolist() == [0, 2, 2, 3, 3, 3, 4, 4, 5, 5]
    assert gt.max_per_cell == 2
    dets, labels, count = _triple()
    p = E.pack_eval_inputs(dets, labels, count, gt, IMG_IDS, CAT_IDS, 'coco')
    assert p.gt_boxes.dtype == torch.float64 and p.gt_off.tolist() == gt.off.tolist() and p.max_gt_per_cell == 2


def test_voc_flattening_puts_regular_before_ignore_boxes():
    anns = [dict(bboxes=np.array([[0, 0, 4, 4], [1, 1, 5, 5]], np.float32), labels=np.array([1, 0]),
                 bboxes_ignore=np.array([[2, 2, 6, 6]], np.float32), labels_ignore=np.array([1])),
            dict(bboxes=np.zeros((0, 4), np.float32), labels=np.zeros(0, np.int64)),
            dict(bboxes=np.array([[3, 3, 9, 9]], np.float32), labels=np.array([1]),
                 bboxes_ignore=np.array([[0, 0, 1, 1]], np.float32), labels_ignore=np.array([0]))]
    gt = E.flatten_annotations(anns, range(3), range(2), 'voc')
    assert gt.boxes.tolist() == [[1., 1., 5., 5.], [0., 0., 1., 1.], [0., 0., 4., 4.], [2., 2., 6., 6.], [3., 3., 9., 9.]]
    assert gt.ignore.tolist() == [0, 1, 0, 1, 0]
    assert gt.off.tolist() == [0, 1, 1, 2, 4, 4, 5]


def test_empty_inputs():
    p = E.pack_eval_inputs(torch.zeros(3, 1, 5), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                           [[], [], []], IMG_IDS, CAT_IDS, 'coco')
    assert p.det_boxes.shape == (0, 4) and p.perm.numel() == 0 and p.det_off.tolist() == [0] * 10
    assert p.gt_boxes.shape == (0, 4) and p.gt_off.tolist() == [0] * 10 and p.max_gt_per_cell == 0
